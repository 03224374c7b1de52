"""Is the gfx950 device code of some kernel files the same in two source trees?

    python tools/kernel_isa_ab.py OTHER_CSRC envelope_kernels.hip quantile_kernels.hip [--rename 'REGEX=TEXT' ...]

Compiles every named file of elodin_amd/csrc in OTHER_CSRC (a checkout of another commit) and in this tree with the library's
flags, disassembles the device code (elodin_amd/isa_check.py) and compares per kernel: the instruction stream, and the register /
LDS / scratch figures of -Rpass-analysis=kernel-resource-usage.  --rename normalises mangled names that differ on purpose (an
argument type renamed).  No GPU is involved.  Exit status 1 when anything differs."""
import argparse
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from elodin_amd.isa_check import disassemble, kernels  # noqa: E402

FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage"]


def device_code(csrc: Path, name: str, norm, tmp: str):
    """-> ({kernel: disassembly lines}, {kernel: resource remarks})"""
    obj = Path(tmp) / f"{abs(hash(str(csrc)))}_{name}.o"
    r = subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "-c", name, "-o", str(obj)], cwd=csrc, capture_output=True, text=True, check=True)
    figures, cur = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", ln)
        if m:
            cur = figures.setdefault(norm(m.group(1)), [])
            continue
        m = re.search(r"remark: +((?:TotalSGPRs|VGPRs|AGPRs|ScratchSize|LDS Size|Occupancy|SGPRs Spill|VGPRs Spill|Dynamic Stack).*?)(?: \[-Rpass.*)?$", ln)
        if m and cur is not None:
            cur.append(m.group(1).strip())
    return {norm(k): [norm(x) for x in v] for k, v in kernels(disassemble(obj)).items()}, figures


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("other_csrc", type=Path)
    ap.add_argument("files", nargs="+")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=TEXT")
    args = ap.parse_args()
    renames = [r.split("=", 1) for r in args.rename]

    def norm(s: str) -> str:
        for pattern, text in renames:
            s = re.sub(pattern, text, s)
        return s
    same = True
    with tempfile.TemporaryDirectory() as tmp:
        for name in args.files:
            a, fa = device_code(args.other_csrc, name, norm, tmp)
            b, fb = device_code(ROOT / "elodin_amd" / "csrc", name, norm, tmp)
            if set(a) != set(b) or set(fa) != set(fb):
                same = False
                print(f"{name}: the kernel sets differ: {sorted(set(a) ^ set(b) | set(fa) ^ set(fb))}")
            for k in sorted(set(a) & set(b)):
                ok = a[k] == b[k] and fa.get(k) == fb.get(k)
                same &= ok
                print(f"{'same     ' if ok else 'DIFFERENT'} {len(b[k]):5d} lines  {'; '.join(fb.get(k, []))}  {k}")
    print("identical device code" if same else "the device code differs")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
