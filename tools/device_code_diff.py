"""Compares the gfx950 device code of two builds of the library, kernel by kernel (CPU; every host-only change needs it).

  python tools/device_code_diff.py LIB_A LIB_B

The two libraries hold the same device code when they have the same set of code symbols, every symbol's instruction text is
identical once the address column is removed, and every kernel descriptor states the same registers, LDS, scratch and spill
counts.  Prints one line with the kernel count and exits 0, or lists what differs and exits 1."""
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "semantic-superpoint_amd"))
import hipbuild  # noqa: E402

FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
          ".vgpr_spill_count", ".sgpr_spill_count")


def device_code(lib_path):
    """({code symbol: instruction text without addresses}, {kernel symbol: {descriptor field: value}})"""
    with tempfile.TemporaryDirectory(prefix="ssp_diff_") as tmp:
        dis, notes = hipbuild.disassemble(lib_path, tmp)
    parts = re.split(r"^[0-9a-f]{16} <([^>]+)>:\n", dis, flags=re.M)
    code = {parts[i]: re.sub(r"//\s*[0-9A-Fa-f]+:", "//", parts[i + 1]) for i in range(1, len(parts), 2)}
    meta = {}
    for blk in re.split(r"\n\s+- (?=\.agpr_count:)", notes)[1:]:
        m = re.search(r"\.symbol:\s+(\S+?)\.kd", blk)
        if m:
            meta[m.group(1)] = {f: int(re.search(r"%s:\s+(\d+)" % re.escape(f), blk).group(1)) for f in FIELDS}
    return code, meta


def differences(lib_a, lib_b):
    (code_a, meta_a), (code_b, meta_b) = device_code(lib_a), device_code(lib_b)
    out = ["only in %s: %s" % (lib, s) for lib, x, y in ((lib_a, code_a, code_b), (lib_b, code_b, code_a)) for s in sorted(set(x) - set(y))]
    out += ["kernel descriptor only in %s: %s" % (lib, s) for lib, x, y in ((lib_a, meta_a, meta_b), (lib_b, meta_b, meta_a))
            for s in sorted(set(x) - set(y))]
    out += ["instructions differ: %s" % s for s in sorted(set(code_a) & set(code_b)) if code_a[s] != code_b[s]]
    out += ["descriptor differs: %s %s -> %s" % (s, meta_a[s], meta_b[s]) for s in sorted(set(meta_a) & set(meta_b)) if meta_a[s] != meta_b[s]]
    return out, len(meta_a), len(code_a)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 2:
        sys.exit(__doc__)
    diffs, n_kernels, n_symbols = differences(*argv)
    for d in diffs:
        print(d)
    if diffs:
        sys.exit(1)
    print("identical device code: %d kernels (%d code symbols), instruction text and descriptors" % (n_kernels, n_symbols))


if __name__ == "__main__":
    main()
