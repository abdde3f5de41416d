"""Records the argument contract of lib.py's read-out and geometry wrappers (tests/test_lib_arguments_cpu.py), on the CPU.

  python tools/record_lib_contract.py PACKAGE_DIR [--out FILE]      case id -> "accepted" or [exception class, message], grouped by
                                                                    operator, a case per line
  python tools/record_lib_contract.py PACKAGE_DIR --time [--against OTHER_DIR]
                                                                    host microseconds of five accepted calls up to the device guard
                                                                    (the two packages in turn, the fastest of 21 windows of 500 calls)

PACKAGE_DIR is a `semantic-superpoint_amd/` directory: this tree's, or that of a `git worktree` of another commit, whose
outcomes can then be diffed against the committed tests/lib_argument_contract.json.  The cases come from the test module of
THIS tree.  No GPU and no built library are needed."""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load_package(path, name="ssp_contract_pkg"):
    """the package directory `path` imported under a private name (the alias package's recipe)"""
    path = os.path.abspath(path)
    pkg = types.ModuleType(name)
    pkg.__path__, pkg.__file__, pkg.__package__ = [path], os.path.join(path, "__init__.py"), name
    sys.modules[pkg.__name__] = pkg
    with open(pkg.__file__) as f:
        exec(compile(f.read(), pkg.__file__, "exec"), pkg.__dict__)
    return pkg.lib


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("package_dir")
    ap.add_argument("--out", default=None, help="default: tests/lib_argument_contract.json of this tree")
    ap.add_argument("--time", action="store_true", help="time the accepted calls instead of recording")
    ap.add_argument("--against", default=None, help="with --time: a second package directory, timed in turn with the first")
    args = ap.parse_args(argv)
    from tests import test_lib_arguments_cpu as T
    lib = load_package(args.package_dir)
    T.install(lib, setattr)
    if args.time:
        libs = {args.package_dir: lib}
        if args.against:
            libs[args.against] = load_package(args.against, "ssp_contract_other")
            T.install(libs[args.against], setattr)
        res = {}
        for name in ("op_epipolar_ransac", "op_two_view_pose", "op_pose_chain", "op_pnp_ransac", "op_bundle_adjust"):
            kwargs, best = T.OPERATORS[name][0](1, T.CAP), {}
            for _ in range(21):
                for tag, one in libs.items():
                    fn = getattr(one, name)
                    assert T.outcome(fn, kwargs) == "accepted", name
                    t0 = time.perf_counter()
                    for _ in range(500):
                        try:
                            fn(**kwargs)
                        except T.Reached:
                            pass
                    best[tag] = min(best.get(tag, 1e9), (time.perf_counter() - t0) / 500 * 1e6)
            res[name] = {tag: round(us, 2) for tag, us in best.items()}
        print(json.dumps(res))
        return
    contract = {cid: T.outcome(getattr(lib, name), kwargs) for cid, name, kwargs, _ in T.cases()}
    out = args.out or T.CONTRACT
    with open(out, "w") as f:
        f.write(T.dump_contract(contract))
    n_ok = sum(v == "accepted" for v in contract.values())
    print("%d cases (%d accepted, %d refused) -> %s" % (len(contract), n_ok, len(contract) - n_ok, out))


if __name__ == "__main__":
    main()
