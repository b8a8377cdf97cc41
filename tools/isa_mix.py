"""Static instruction mix of the IB node bodies, per basic block. Needs the compiler only, no GPU.

  python tools/isa_mix.py KERNEL [KERNEL ...] [--asm FILE.s] [--min-reads N] [--top N] [--reads N ...] [--sum LABEL[*N] ...]
                           [-D NAME=VALUE ...]

Compiles csrc/ib_kernels.hip to gfx950 assembly with the build's flags (_build.py FLAGS; --asm reuses or
writes FILE.s instead of a temporary) and prints, for every kernel whose name, written as in the source, contains KERNEL
(e.g. "ib_cn_fast<8,false,1>"), its register / private-segment figures and one line per basic block
with at least --min-reads LDS lookups: the ds_read_u8 count (and, where a body ends its chains in the composite
step, the ds_read_b32 count beside it; a lookup is either), the VALU count, VALU per lookup and the VALU
opcode histogram, blocks sorted by lookups (--top N: the first N; --reads: only blocks with these lookup counts,
e.g. the 10 lookups of a degree-3 variable group of 2 codewords). --sum adds up the named blocks of ONE kernel, a
block executed N times as LABEL*N: the instructions one item executes where its body is a loop nest ("LABEL+" is
the code that follows LABEL's branch up to the next label). A node body is straight-line code, so the hot blocks are the
4-codeword (check) / S-codeword (variable) groups of one degree.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from informationbottleneckdecodingldpc_amd import _build  # noqa: E402

BRANCH = ("s_branch", "s_cbranch", "s_endpgm", "s_setpc", "s_swappc")
WIDE = "ds_read_b32"   # the composite step's read (the node bodies have no other 4-byte LDS read)


def reads(ops):
    """(ds_read_u8, ds_read_b32) of a block"""
    return sum(op == "ds_read_u8" for op in ops), sum(op == WIDE for op in ops)


def rd(n8, n32):
    return f"ds_read_u8 {n8:4d}" + (f" + b32 {n32:3d}" if n32 else "")


def pretty(name):
    """ib_cn_fast<8,false,1> from _ZN3ibl10ib_cn_fastILi8ELb0ELi1EEEvNS_10IbFastArgsE (integer / bool template
    arguments are all these kernels have)"""
    m = re.match(r"_ZN3ibl\d+(\w+?)(?:I((?:L[ib]\d+E)+)E)?Ev", name)
    if not m:
        return name
    args = [("true" if v != "0" else "false") if t == "b" else v for t, v in re.findall(r"L([ib])(\d+)E", m.group(2) or "")]
    return m.group(1) + (f"<{','.join(args)}>" if args else "")


def compile_asm(path, defines):
    src = os.path.join(_build.CSRC, "ib_kernels.hip")
    cmd = [_build.HIPCC, *_build.FLAGS, *_build.SRC_FLAGS.get("ib_kernels.hip", []), *[f"-D{d}" for d in defines],
           "--cuda-device-only", "-S", src, "-o", path]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit("hipcc failed")


def kernels(lines):
    """{mangled name: (first line, last line)} of the functions of an assembly file"""
    out, cur = {}, None
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z\w+):", l)
        if m:
            cur = (m.group(1), i)
        elif l.startswith(".Lfunc_end") and cur:
            out[cur[0]] = (cur[1], i)
            cur = None
    return out


def blocks(body):
    """[(label, [opcode, ...])]: a block ends at a label or after a branch"""
    out, label, ops = [], "entry", []
    for l in body:
        m = re.match(r"^(\.LBB\w+):", l)
        if m:
            if ops:
                out.append((label, ops))
            label, ops = m.group(1), []
            continue
        m = re.match(r"^\s+([a-z][a-z_0-9]+)(\s|$)", l)
        if not m:
            continue
        ops.append(m.group(1))
        if m.group(1).startswith(BRANCH):
            out.append((label, ops))
            label, ops = label + "+", []
    if ops:
        out.append((label, ops))
    return out


def meta(lines, name):
    """figures of the kernel's .amdhsa descriptor"""
    keys = ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size")
    got, on = {}, False
    for l in lines:
        l = l.strip()
        if l.startswith(".amdhsa_kernel"):
            on = l.split()[1] == name
        elif on:
            for k in keys:
                m = re.match(rf"\.amdhsa_{k}\s+(\d+)", l)
                if m:
                    got[k] = int(m.group(1))
            if l.startswith(".end_amdhsa_kernel"):
                break
    return got


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("kernel", nargs="+")
    ap.add_argument("--asm", help="assembly file: used if it exists, else written")
    ap.add_argument("--min-reads", type=int, default=8)
    ap.add_argument("--top", type=int, default=0)
    ap.add_argument("--reads", type=int, nargs="*", default=[])
    ap.add_argument("--sum", nargs="*", default=[])
    ap.add_argument("-D", dest="defines", action="append", default=[])
    a = ap.parse_args()
    tmp = None
    path = a.asm
    if not path:
        tmp = tempfile.TemporaryDirectory()
        path = os.path.join(tmp.name, "ib_kernels.s")
    if not os.path.exists(path):
        compile_asm(path, a.defines)
    lines = open(path).read().splitlines()
    ks = kernels(lines)
    names = list(ks)
    dem = [pretty(n) for n in names]
    for want in a.kernel:
        hit = [(n, d) for n, d in zip(names, dem) if want.replace(" ", "") in d]
        if not hit:
            raise SystemExit(f"no kernel matches {want!r}")
        for n, d in hit:
            lo, hi = ks[n]
            bl = blocks(lines[lo + 1:hi])
            m = meta(lines, n)
            tot_v = sum(op.startswith("v_") for _, ops in bl for op in ops)
            tot_r, tot_w = (sum(x) for x in zip(*(reads(ops) for _, ops in bl)))
            print(f"== {d}")
            print(f"   vgpr {m.get('next_free_vgpr')} sgpr {m.get('next_free_sgpr')} private "
                  f"{m.get('private_segment_fixed_size')} B; static totals: ds_read_u8 {tot_r}, {WIDE} {tot_w}, VALU {tot_v}")
            if a.sum:
                by, nr, nw, nv = dict(bl), 0, 0, 0
                for term in a.sum:
                    lab, _, n = term.partition("*")
                    nr += int(n or 1) * reads(by[lab])[0]
                    nw += int(n or 1) * reads(by[lab])[1]
                    nv += int(n or 1) * sum(op.startswith("v_") for op in by[lab])
                print(f"   sum of {' '.join(a.sum)}: {rd(nr, nw)}  VALU {nv}  VALU/lookup {nv / (nr + nw):.2f}")
                continue
            rows = []
            for label, ops in bl:
                nr, nw = reads(ops)
                if nr + nw < a.min_reads:
                    continue
                hist = {}
                for op in ops:
                    if op.startswith("v_"):
                        hist[op] = hist.get(op, 0) + 1
                rows.append((nr + nw, sum(hist.values()), label, hist, nr, nw))
            rows.sort(key=lambda r: (-r[0], r[2]))
            if a.reads:
                rows = [r for r in rows if r[0] in a.reads]
            if a.top:
                rows = rows[:a.top]
            for n, nv, label, hist, nr, nw in rows:
                h = " ".join(f"{k[2:]}:{v}" for k, v in sorted(hist.items(), key=lambda kv: -kv[1]))
                print(f"   {label:<12} {rd(nr, nw)}  VALU {nv:4d}  VALU/lookup {nv / max(n, 1):5.2f}  | {h}")
    if tmp:
        tmp.cleanup()


if __name__ == "__main__":
    main()
