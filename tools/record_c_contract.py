"""Records the refusal contract of the operator-level C entry points (tests/test_c_refusals_cpu.py), on the CPU.

  python tools/record_c_contract.py LIBRARY [--out FILE]     case id -> [return value, class, message], grouped by entry point,
                                                             a case per line (default: tests/c_refusal_contract.json of this tree)

LIBRARY is a built libssp_hip.so: this tree's, or that of another commit (built into a path of its own), whose answers can then be
diffed against the committed contract.  The cases, the signatures and the parameter structs come from THIS tree.  The machine must
have no GPU: an accepted call is let through to its first device call, which has to fail."""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("library")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import torch
    if torch.cuda.is_available():
        sys.exit("a device is present: the accepted calls would launch on NULL pointers")
    from semantic_superpoint_amd import lib as L
    from tests import test_c_refusals_cpu as T
    lib = ctypes.CDLL(os.path.abspath(args.library))
    for name, (argtypes, restype) in L.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = argtypes, restype
    contract = T.record(L, lib)
    out = args.out or T.CONTRACT
    with open(out, "w") as f:
        f.write(T.dump_contract(contract))
    n_ok = sum(v[0] == -2 for v in contract.values())
    print("%d cases of %d entry points (%d let through, %d refused or answered) -> %s"
          % (len(contract), len({c.split("/")[0] for c in contract}), n_ok, len(contract) - n_ok, out))


if __name__ == "__main__":
    main()
