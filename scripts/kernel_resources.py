"""profiles/kernel_resources.txt from the built library: every kernel's VGPRs, SGPRs, static LDS and scratch, read from the notes of the
gfx950 code object inside isocon_amd/lib/libisocon_hip.so (llvm-objcopy, clang-offload-bundler, llvm-readelf of the ROCm LLVM; c++filt).
Offline: no GPU is needed.  The header lines of the existing file are kept, with the kernel counts brought up to date.
Usage: python scripts/kernel_resources.py [--so file] [--out file]"""
import argparse, os, re, shutil, subprocess, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the LLVM tools of the ROCm installation whose hipcc is on the PATH (or of $ROCM_PATH)
LLVM = os.path.join(os.environ.get("ROCM_PATH") or os.path.dirname(os.path.dirname(os.path.realpath(shutil.which("hipcc")))), "llvm", "bin")

ap = argparse.ArgumentParser()
ap.add_argument("--so", default=os.path.join(ROOT, "isocon_amd", "lib", "libisocon_hip.so"))
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kernel_resources.txt"))
args = ap.parse_args()

with tempfile.TemporaryDirectory() as tmp:
    fatbin, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "co")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", args.so, fatbin])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fatbin, "--output=" + co])
    notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
rows = []
for blk in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
    field = lambda k: re.search(r"\.%s:\s+(\S+)" % k, blk).group(1)
    name = subprocess.check_output(["c++filt", field("name")], text=True).strip()
    name = re.sub(r"\((?!anonymous namespace\)).*\)$", "", re.sub(r"^void ", "", name))          # without the return type and the argument list
    rows.append((name, int(field("vgpr_count")), int(field("sgpr_count")), int(field("group_segment_fixed_size")), int(field("private_segment_fixed_size"))))
rows.sort()
with open(args.out) as f:
    head = [ln for ln in f if ln.startswith("#")]
head = [re.sub(r"^# \d+ kernels, \d+ with scratch", "# %d kernels, %d with scratch" % (len(rows), sum(1 for r in rows if r[4])), ln) for ln in head]
with open(args.out, "w") as f:
    f.writelines(head)
    f.write("%-110s%6s%6s%9s%9s\n" % ("kernel", "vgpr", "sgpr", "lds B", "scratch"))
    for r in rows:
        f.write("%-110s%6d%6d%9d%9d\n" % r)
print("%d kernels, %d with scratch -> %s" % (len(rows), sum(1 for r in rows if r[4]), args.out))
