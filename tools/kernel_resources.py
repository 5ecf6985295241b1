"""Per-kernel resources of a built library's gfx950 code objects: VGPR, AGPR and
SGPR counts, private-segment (scratch) and LDS bytes from the code objects'
metadata notes, and the kernel symbol's code size from their symbol tables.

    python tools/kernel_resources.py LIB            the table of LIB
    python tools/kernel_resources.py OLD NEW        the kernels that differ, as JSON
                                                    (exit status 1 if any does)
    python tools/kernel_resources.py OLD NEW --json FILE   also written to FILE

A change that only moves code between translation units must leave the table as
it was: the same kernel names, none in two code objects, the same figures.
The code objects are extracted as tools/long_branch_check.py does."""
import json
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from long_branch_check import LLVM, code_objects  # noqa: E402

READELF = os.path.join(LLVM, "llvm-readelf")
FIELDS = {".vgpr_count": "vgpr", ".agpr_count": "agpr", ".sgpr_count": "sgpr",
          ".private_segment_fixed_size": "scratch", ".group_segment_fixed_size": "lds"}
ENTRY = re.compile(r"^  - (\.\w+):\s*(.*)$")  # first key of a kernel's metadata entry
KEY = re.compile(r"^    (\.\w+):\s*(.*)$")    # its other top-level keys (arguments sit deeper)


def note_kernels(co):
    """{kernel: {vgpr, agpr, sgpr, scratch, lds}} from the amdhsa.kernels note of one code object"""
    out = subprocess.check_output([READELF, "--notes", co], text=True)
    kernels, cur, inside = {}, None, False

    def close(entry):
        if entry and ".name" in entry:
            kernels[entry[".name"]] = {v: int(entry[k]) for k, v in FIELDS.items()}

    for line in out.splitlines():
        if line.startswith("amdhsa.kernels:"):
            inside = True
            continue
        if not inside:
            continue
        if line and not line.startswith(" "):  # the next top-level key ends the list
            inside = False
            continue
        m = ENTRY.match(line)
        if m:
            close(cur)
            cur = {}
        else:
            m = KEY.match(line)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2).strip().strip("'\"")
    close(cur)
    return kernels


def code_sizes(co):
    """{function symbol: bytes} of one code object"""
    out = subprocess.check_output([READELF, "-sW", co], text=True)
    sizes = {}
    for line in out.splitlines():
        parts = line.split()
        if len(parts) >= 8 and parts[0].endswith(":") and parts[3] == "FUNC":
            sizes[parts[7]] = int(parts[2], 0)
    return sizes


def table(lib):
    """({kernel: figures}, [kernels found in more than one code object])"""
    kernels, twice = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(lib, tmp):
            sizes = code_sizes(co)
            for name, fig in note_kernels(co).items():
                if name in kernels:
                    twice.append(name)
                fig["code"] = sizes.get(name, -1)
                kernels[name] = fig
    return kernels, sorted(twice)


def diff(old, new):
    a, a2 = table(old)
    b, b2 = table(new)
    return {"kernels_old": len(a), "kernels_new": len(b),
            "only_old": sorted(set(a) - set(b)), "only_new": sorted(set(b) - set(a)),
            "in_two_code_objects_old": a2, "in_two_code_objects_new": b2,
            "changed": {k: {"old": a[k], "new": b[k]} for k in sorted(set(a) & set(b)) if a[k] != b[k]}}


def main():
    args = sys.argv[1:]
    out = None
    if "--json" in args:
        i = args.index("--json")
        out = args[i + 1]
        del args[i:i + 2]
    if len(args) == 1:
        kernels, twice = table(args[0])
        print("%6s %5s %5s %8s %7s %8s  kernel" % ("vgpr", "agpr", "sgpr", "scratch", "lds", "code"))
        for k in sorted(kernels):
            f = kernels[k]
            print("%6d %5d %5d %8d %7d %8d  %s" % (f["vgpr"], f["agpr"], f["sgpr"], f["scratch"], f["lds"], f["code"], k))
        for k in twice:
            print("in two code objects: " + k)
        sys.exit(1 if twice else 0)
    if len(args) != 2:
        sys.exit(__doc__)
    d = diff(args[0], args[1])
    text = json.dumps(d, indent=1)
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")
    clean = not (d["only_old"] or d["only_new"] or d["changed"] or d["in_two_code_objects_new"])
    sys.exit(0 if clean else 1)


if __name__ == "__main__":
    main()
