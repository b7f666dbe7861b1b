"""Per-kernel resource figures of a built library's gfx950 code objects (no GPU needed):
VGPRs, AGPRs, SGPRs, static LDS, scratch and spill counts from the code object notes, as
tests/test_code_object.py reads them.

  python tools/kernel_figures.py LIB [--match REGEX] [--against OLD_LIB]

With --against, kernels are paired by mangled name after `--strip REGEX` is removed
from LIB's names (e.g. a trailing template argument that OLD_LIB's lack), and every
pair is printed with "same" or the differing fields."""
import argparse
import os
import re
import subprocess
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
FIELDS = (("vgpr", r"\.vgpr_count:\s+(\d+)"), ("agpr", r"\.agpr_count:\s+(\d+)"), ("sgpr", r"\.sgpr_count:\s+(\d+)"),
          ("lds", r"\.group_segment_fixed_size:\s+(\d+)"), ("scratch", r"\.private_segment_fixed_size:\s+(\d+)"),
          ("vspill", r"\.vgpr_spill_count:\s+(\d+)"), ("sspill", r"\.sgpr_spill_count:\s+(\d+)"))


def figures(lib):
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fat.bin")
        subprocess.run(["objcopy", "--dump-section", ".hip_fatbin=%s" % fat, lib], check=True, capture_output=True)
        data = open(fat, "rb").read()
        offs = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
        for i, o in enumerate(offs):
            part, co = os.path.join(tmp, "b%d" % i), os.path.join(tmp, "c%d.o" % i)
            open(part, "wb").write(data[o:offs[i + 1] if i + 1 < len(offs) else len(data)])
            subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--unbundle",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=%s" % part, "--output=%s" % co],
                           check=True, capture_output=True)
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True,
                                   text=True).stdout
            for block in notes.split("  - .agpr_count:")[1:]:
                block = ".agpr_count:" + block
                name = re.search(r"\.name:\s+(\S+)", block).group(1)
                out[name] = {k: int(re.search(rx, block).group(1)) for k, rx in FIELDS}
    return out


def fmt(f):
    return " ".join("%s=%d" % (k, f[k]) for k, _ in FIELDS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lib")
    ap.add_argument("--match", default=".")
    ap.add_argument("--against")
    ap.add_argument("--strip", default=None)
    a = ap.parse_args()
    new = {k: v for k, v in figures(a.lib).items() if re.search(a.match, k)}
    if not a.against:
        for k in sorted(new):
            print(k, fmt(new[k]))
        return
    key = (lambda n: re.sub(a.strip, "", n)) if a.strip else (lambda n: n)
    old = {k: (k, v) for k, v in figures(a.against).items() if re.search(a.match, k)}
    paired = set()
    for k in sorted(new):
        if key(k) in old:
            paired.add(key(k))
            ok, ov = old[key(k)]
            diff = [f for f, _ in FIELDS if ov[f] != new[k][f]]
            print(ok, "|", fmt(ov), "|", "same" if not diff else "DIFFERS " + " ".join(
                "%s %d->%d" % (f, ov[f], new[k][f]) for f in diff))
        else:
            print("new", k, "|", fmt(new[k]))
    for k in sorted(set(old) - paired):
        print("gone", old[k][0])


if __name__ == "__main__":
    main()
