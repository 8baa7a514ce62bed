#!/usr/bin/env python3
"""Static instruction counts of the loops of one kernel in a gfx950 assembly listing.

    hipcc --offload-arch=gfx950 -O2 -std=c++17 -Iinclude -mllvm -pragma-unroll-threshold=1000000 \\
        -DALQP_QUAD_F32 '-DALQP_FOR_EACH_DIMS(X)=X(13,4)' --cuda-device-only -S \\
        deq-mpc-corl_amd/csrc/alqp_quad.hip -o quad_f32.s
    tools/loop_inst_count.py quad_f32.s k_solve_lin_quad Li13ELi4ELb0ENS_5NoDyn --min=600

Loops are the natural loops of the kernel's control-flow graph (blocks laid out behind the back branch included; blocks
laid out in front of the loop header are not followed: an approximation that holds for hipcc's layout of these kernels); the
kernels' stage loops are the big ones (the fused solve has the forward sweep's first, then the backward sweep's).
Prints, per loop of at least MIN instructions (--min=MIN, default 300) in every kernel whose mangled name holds all the
given substrings: all instructions, VALU (v_*), v_mov_b32_dpp, every *_dpp, fma-type (v_fma*, v_fmac*, v_pk_fma*),
v_cndmask, accumulator-register moves, s_nop."""
import re
import sys


def loops(lines):
    """Natural loops of the listing: [(first line of the header block, [lines of the loop's blocks])], one per header."""
    # basic blocks: a label starts one, a branch ends one
    starts = {0}
    label_at = {}
    for i, ln in enumerate(lines):
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            label_at[m.group(1)] = i
            starts.add(i)
        if re.match(r"^\s+s_c?branch", ln) or re.match(r"^\s+s_endpgm", ln):
            starts.add(i + 1)
    starts = sorted(x for x in starts if x < len(lines))
    block_of = {}
    for bi, a in enumerate(starts):
        for i in range(a, starts[bi + 1] if bi + 1 < len(starts) else len(lines)):
            block_of[i] = bi
    succ = [[] for _ in starts]
    for bi, a in enumerate(starts):
        e = (starts[bi + 1] if bi + 1 < len(starts) else len(lines)) - 1
        last = next((lines[i] for i in range(e, a - 1, -1) if re.match(r"^\s+[a-z]", lines[i])), "")
        m = re.match(r"^\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", last)
        if m and m.group(1) in label_at:
            succ[bi].append(block_of[label_at[m.group(1)]])
        if not re.match(r"^\s+(s_branch|s_endpgm|s_setpc)", last) and bi + 1 < len(starts):
            succ[bi].append(bi + 1)
    pred = [[] for _ in starts]
    for bi, ss in enumerate(succ):
        for t in ss:
            pred[t].append(bi)
    by_header = {}
    for bi, ss in enumerate(succ):
        for h in ss:
            if h <= bi:   # back edge (blocks are in layout order; the kernels' loops are reducible)
                body = by_header.setdefault(h, {h})
                stack = [bi]
                while stack:
                    x = stack.pop()
                    if x in body or x < h:
                        continue
                    body.add(x)
                    stack.extend(pred[x])
    out = []
    for h, body in sorted(by_header.items()):
        ls = []
        for bi in sorted(body):
            ls += range(starts[bi], starts[bi + 1] if bi + 1 < len(starts) else len(lines))
        out.append((starts[h], ls))
    return out


def count(body):
    ins = [ln.split()[0] for ln in body if re.match(r"^\s+[a-z]", ln) and not ln.lstrip().startswith((".", ";"))]
    c = {"all": len(ins)}
    c["valu"] = sum(1 for x in ins if x.startswith("v_") and x != "v_nop")
    c["mov_dpp"] = sum(1 for x in ins if x == "v_mov_b32_dpp")
    c["dpp"] = sum(1 for x in ins if x.endswith("_dpp"))
    c["fma"] = sum(1 for x in ins if re.match(r"v_(pk_)?fma", x))
    c["cndmask"] = sum(1 for x in ins if x.startswith("v_cndmask"))
    c["acc_mov"] = sum(1 for x in ins if x.startswith("v_accvgpr"))
    c["s_nop"] = sum(1 for x in ins if x == "s_nop")
    return c


def main():
    path, subs = sys.argv[1], [a for a in sys.argv[2:] if not a.startswith("--min=")]
    mn = next((int(a[6:]) for a in sys.argv[2:] if a.startswith("--min=")), 300)
    txt = open(path).read().split("\n")
    start = None
    for i, ln in enumerate(txt):
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            start = (m.group(1), i)
        if start and re.match(r"^\.Lfunc_end\d+:", ln):
            name, a = start
            if all(s in name for s in subs):
                print(name)
                body = txt[a:i + 1]
                for la, ls in loops(body):
                    c = count([body[x] for x in ls])
                    if c["all"] >= mn:
                        print("  loop at +%d: " % la + " ".join(f"{k}={v}" for k, v in c.items()))
            start = None


if __name__ == "__main__":
    main()
