"""Static instruction counts of one kernel in a gfx950 assembly file
(hipcc --cuda-device-only -S): the whole kernel, every loop (a label with a backward
branch to it) and every sched_barrier-delimited region, each with its opcode census.

    python scripts/isa_loop_counts.py FILE.s KERNEL_SUBSTRING [--top N] [--ops REGEX]

The Jacobi sweep loop (jacobi_os) is the ~1.7-1.9 k-instruction loop of hd_layer_kernel<8>.
A backward branch counts as a loop: a cold block that the compiler placed behind a loop and
that branches back to the kernel's start shows up as a larger "loop" spanning it.  --ops limits
the census to the opcodes matching REGEX (default: the ones the layer kernel's
bookkeeping shows up in); --top lists only the N largest loops.
profiles/layerdiet/isa_counts.txt is this script's output for hd_layer_kernel<8,true>.
"""
import argparse
import collections
import re

DEFAULT_OPS = (r"v_fma_f64|v_mul_f64|v_add_f64|v_cmp\w*_f64|v_cndmask_b32|s_and_b64|"
               r"v_rsq_f64|v_rcp_f64|v_accvgpr_\w+|s_cbranch_execz|v_mov_b32|s_mov_b32|"
               r"scratch_\w+")


def kernel_body(text, pat):
    m = next(m for m in re.finditer(r"^(\S+):\s*; @", text, re.M) if pat in m.group(1))
    return m.group(1), text[m.start():text.index(".Lfunc_end", m.start())].split("\n")


def instructions(lines):
    """(line index, opcode) of every instruction, and the line index of every label"""
    ins, labels = [], {}
    for k, line in enumerate(lines):
        t = line.split(";")[0].strip()
        if not t or t.startswith("."):
            m = re.match(r"(\.LBB\w+):", t)
            if m:
                labels[m.group(1)] = k
            continue
        if t.endswith(":"):
            continue
        ins.append((k, t.split()[0]))
    return ins, labels


def census(ops, want):
    c = collections.Counter(o for o in ops if want.fullmatch(o))
    return ", ".join(f"{k} {v}" for k, v in sorted(c.items())) or "-"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("file")
    ap.add_argument("kernel")
    ap.add_argument("--top", type=int, default=4)
    ap.add_argument("--ops", default=DEFAULT_OPS)
    a = ap.parse_args()
    want = re.compile(a.ops)
    name, lines = kernel_body(open(a.file).read(), a.kernel)
    ins, labels = instructions(lines)
    print(f"kernel {name}")
    print(f"whole kernel: {len(ins)} instructions; {census([o for _, o in ins], want)}")

    loops = []
    for k, line in enumerate(lines):
        m = re.match(r"\s*s_cbranch_\w+\s+(\.LBB\w+)|\s*s_branch\s+(\.LBB\w+)", line)
        if m:
            tgt = labels.get(m.group(1) or m.group(2))
            if tgt is not None and tgt < k:
                loops.append((tgt, k))
    loops.sort(key=lambda lk: -sum(1 for i, _ in ins if lk[0] <= i <= lk[1]))
    for lo, hi in loops[:a.top]:
        ops = [o for i, o in ins if lo <= i <= hi]
        print(f"loop lines {lo}-{hi}: {len(ops)} instructions; {census(ops, want)}")

    start, n = 0, 0
    bounds = [k for k, line in enumerate(lines) if "sched_barrier" in line] + [len(lines)]
    for b in bounds:
        ops = [o for i, o in ins if start <= i < b]
        print(f"region {n} lines {start}-{b}: {len(ops)} instructions; "
              f"{census(ops, re.compile(r'v_fma_f64|v_mul_f64|v_add_f64|v_mov_b32|s_mov_b32'))}")
        start, n = b, n + 1


if __name__ == "__main__":
    main()
