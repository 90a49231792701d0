#!/usr/bin/env python3
"""Device code of two source trees, kernel by kernel: what a refactor of the kernel headers may and may not move.
usage: scripts/kernel_diff.py OLD NEW [-- extra hipcc flags]     OLD / NEW: a checkout's root, or a gfx950 code object
Prints one line per kernel and exits 1 if the kernel set or order, a kernel's metadata (registers, LDS, scratch, spills) or its
count of MFMA / vector-memory / ds_* / s_barrier / s_waitcnt instructions differs; every other opcode whose count moved is listed."""
import collections
import re
import subprocess
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from kernel_resources import kernel_resources  # noqa: E402

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
PINNED = ("mfma", "vmem", "ds", "s_barrier", "s_waitcnt")


def code_object(arg, flags, tmp):
    p = Path(arg)
    if p.is_file():
        return p
    co = Path(tmp) / (p.resolve().name + f"_{len(list(Path(tmp).iterdir()))}.co")
    src = p / "voice_activity_detection_amd" / "csrc" / "savad.hip"
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "--no-gpu-bundle-output",
                    "-Wno-unused-value", "-w", *flags, str(src), "-o", str(co)], check=True)
    return co


def pinned_class(op):
    if "mfma" in op:
        return "mfma"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("ds_"):
        return "ds"
    return op if op in ("s_barrier", "s_waitcnt") else None


def kernels(co):
    """[(symbol, [instruction text ...])] in code-object order, kernels only"""
    meta = kernel_resources(co=co)
    text = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "--no-leading-addr", str(co)], check=True, capture_output=True, text=True).stdout
    out, cur = [], None
    for line in text.splitlines():
        sym = re.match(r"^(?:[0-9a-f]+ )?<([^>]+)>:", line)
        if sym:
            cur = [] if sym.group(1) in meta else None
            if cur is not None:
                out.append((sym.group(1), cur, meta[sym.group(1)]))
        elif cur is not None and line.startswith(("\t", " ")) and line.strip() not in ("", "..."):
            cur.append(re.sub(r"\s+", " ", line.split("//")[0].strip()))
    return out


def main():
    args, flags = sys.argv[1:], []
    if "--" in args:
        args, flags = args[:args.index("--")], args[args.index("--") + 1:]
    with tempfile.TemporaryDirectory() as tmp:
        old, new = (kernels(code_object(a, flags, tmp)) for a in args)
    bad = same = 0
    if [k[0] for k in old] != [k[0] for k in new]:
        print("FAIL kernel set / order differs:", sorted({k[0] for k in old} ^ {k[0] for k in new}) or "same set, other order")
        bad += 1
    new_by = {k[0]: k for k in new}
    for name, ins_o, meta_o in old:
        if name not in new_by:
            continue
        _, ins_n, meta_n = new_by[name]
        short = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip().split("(")[0] or name
        if ins_o == ins_n and meta_o == meta_n:
            same += 1
            print(f"identical  {short}")
            continue
        cnt_o, cnt_n = (collections.Counter(i.split(" ")[0] for i in ins) for ins in (ins_o, ins_n))
        pin_o, pin_n = ({c: sum(v for op, v in cnt.items() if pinned_class(op) == c) for c in PINNED} for cnt in (cnt_o, cnt_n))
        moved = {op: (cnt_o[op], cnt_n[op]) for op in sorted(set(cnt_o) | set(cnt_n)) if cnt_o[op] != cnt_n[op]}
        fail = [f"{k} {meta_o[k]}->{meta_n[k]}" for k in meta_o if meta_o[k] != meta_n[k]]
        fail += [f"{c} {pin_o[c]}->{pin_n[c]}" for c in PINNED if pin_o[c] != pin_n[c]]
        bad += bool(fail)
        print(f"{'FAIL     ' if fail else 'differs  '}  {short}: {len(ins_o)}->{len(ins_n)} instructions; " +
              ("; ".join(fail) + "; " if fail else "") +
              ("opcodes " + ", ".join(f"{op} {a}->{b}" for op, (a, b) in moved.items()) if moved else "same opcode counts, other order or operands"))
    print(f"{len(old)} kernels, {same} with identical instruction stream and metadata, {bad} failures")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
