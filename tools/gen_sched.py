"""Generate the IB fast path's per-degree fold schedules (csrc/ib_sched.inc).

The check-node (variable-node) update of one group of S codewords is a DAG of lookup chains
(kernels_template_irreg.cl:205-231 / :151-160, prefix-shared as in ib_kernels.hip):
  CN degree D:  out0 chain  in1 -> B0(.,in2) -> ... -> B_{D-3}(.,in_{D-1})           (D-2 steps)
                P chain     in0 -> B0(.,in1) = P2 -> B1(.,in2) = P3 ... -> out_{D-1}  (D-2 steps)
                chain w     P_w -> B_{w-1}(.,in_{w+1}) -> ... -> out_w, w=1..D-2     (D-1-w steps)
  VN degree D:  out0 chain  V0(c,in1) -> V1(.,in2) -> ... -> out0                    (D-1 steps)
                Q chain     V0(c,in0) = Q1 -> V1(.,in1) = Q2 ... -> out_{D-1}        (D-1 steps)
                chain w     Q_w -> V_w(.,in_{w+1}) -> ... -> out_w, w=1..D-2         (D-1-w steps)
Every chain is a sequence of dependent LDS lookups; chains are independent once their start value
exists, so the critical path is D-2 (CN) / D-1 (VN) steps, not the 25 / 35 of running them one
after another. This script list-schedules the chains onto L concurrent lanes (critical path first)
and emits straight-line code with one SSA name per value (no register copies): each time step
issues the lookups of every running lane for all S sub-slots back to back.

Degree-2 variable fold (the folding unrolled bodies cn_group_fold_ct, check degrees 3..8). The message of a
degree-2 variable to one of its checks is F2(channel, message from its other check): one lookup on a value the
check pass has just computed. The folding bodies append it to the chains of outputs D-2 / D-1 (bit 0 / 1 of the
class FC) as one more link, t' = luc(t, q_ch, 0) with q_ch the v_perm_b32 column term of the variable's channel
word (lane term = lane4c, which holds the slot of the transposed degree-2 table) - the price of any other lookup,
taken while t is still alone in a register.

Composite final step (the unrolled bodies cn_group_fold_cp, check degrees 5..8; DESIGN.md "Composite final step of the
check chains"). For the one check degree whose composite table C(t, m)[y] = F(L(t, m), y) the launch has staged, the
chains of outputs 0 .. D-3 take their last two steps, "-> L(., in_{D-2}) -> F(., in_{D-1})", as one: a ds_read_b32 of
the half y >> 3 of C(t, in_{D-2}) (IBL_LUK: column term qk, shared by those chains) and, with the packing one step
later, nibble y & 7 of it (IBL_PKK: shift sh). Outputs D-2 and D-1 and the fold links are as before.

Column fetches (one ds_read_b64 of a table's whole column for the inputs that meet the same table in every chain)
were measured on DVB-S2, B=8192, i_max=50, and lost: 170.9k -> 140.9k cw/s (CN 0.464 -> 0.622 ms, VN 0.478 -> 0.526
ms). The code last stood in the parent of the commit that removed it (DESIGN.md "Retired experiment arms").

usage: python tools/gen_sched.py [S_cn L_cn S_vn L_vn] > informationbottleneckdecodingldpc_amd/csrc/ib_sched.inc
(measured on DVB-S2: CN S=4 L=2, VN S=2 L=4)
       python tools/gen_sched.py --unrolled [S_cn L_cn S_vn L_vn] > informationbottleneckdecodingldpc_amd/csrc/ib_unrolled.inc
(the unrolled bodies of the degree <= 8 kernels, see "Unrolled bodies" below)
"""
import sys

KMAXD = 16


def slot_off(l):   # csrc/common.h: quad l >> 2 in super-region l >> 3, half (l >> 2) & 1, byte l & 3
    return (l >> 3) * 65536 + ((l >> 2) & 1) * 128 + (l & 3)


def cn_chains(D):
    def st(j, l):
        sl = "0u" if j == D - 1 else ("fbase" if l == D - 3 else f"{slot_off(l)}u")
        return ("q", j, sl, l)
    ch = [dict(id="o0", start=("nib", 1), steps=[st(j, j - 2) for j in range(2, D)], out=0),
          dict(id="P", start=("nib", 0), steps=[st(w, w - 1) for w in range(1, D - 1)], out=D - 1)]
    for w in range(1, D - 1):
        s0 = ("nib", 0) if w == 1 else ("val", "P", w - 2)              # P_w = P chain after step w-2
        ch.append(dict(id=f"c{w}", start=s0, steps=[st(j, j - 2) for j in range(w + 1, D)], out=w))
    return ch


def cn_chains_composite(D):
    """cn_chains with the last two steps of outputs 0 .. D-3 as one composite step ("k": a read of C_D at
    (t, in_{D-2}), nibble in_{D-1} of it; DESIGN.md "Composite final step")."""
    ch = cn_chains(D)
    for c in ch:
        if c["out"] <= D - 3:
            assert len(c["steps"]) >= 2 and [st[1] for st in c["steps"][-2:]] == [D - 2, D - 1]
            c["steps"][-2:] = [("k", D - 2, None, None)]
    return ch


def vn_chains(D):
    def st(op, j, l):
        sl = "0u" if j == D - 1 else ("fbase" if l == D - 2 else f"{slot_off(l)}u")
        return (op, j, sl, l)
    ch = [dict(id="o0", start=("chan",), steps=[st("c", 1, 0)] + [st("q", j, j - 1) for j in range(2, D)], out=0),
          dict(id="Q", start=("chan",), steps=[st("c", 0, 0)] + [st("q", w, w) for w in range(1, D - 1)], out=D - 1)]
    for w in range(1, D - 1):
        ch.append(dict(id=f"c{w}", start=("val", "Q", w - 1),           # Q_w = Q chain after step w-1
                       steps=[st("q", j, j - 1) for j in range(w + 1, D)], out=w))
    return ch


def vn_chains_composite(D):
    """vn_chains with the last two steps of outputs 0 .. D-3, "-> V_{D-3}(., in_{D-2}) -> final(., in_{D-1})", as one
    composite step ("k", as cn_chains_composite; DESIGN.md "Composite final step of the variable chains")."""
    ch = vn_chains(D)
    for c in ch:
        if c["out"] <= D - 3:
            assert len(c["steps"]) >= 2 and [st[1] for st in c["steps"][-2:]] == [D - 2, D - 1]
            assert [st[3] for st in c["steps"][-2:]] == [D - 3, D - 2]
            c["steps"][-2:] = [("k", D - 2, None, None)]
    return ch


def schedule(chains, L):
    """List scheduling: returns [(time, [(chain, step_index), ...]), ...]."""
    by_id = {c["id"]: c for c in chains}
    # downstream weight: a prefix chain gates every suffix chain -> schedule it first
    for c in chains:
        c["prio"] = len(c["steps"]) + (100 if c["id"] in ("P", "Q") else 0)
    ready_at = {}
    for c in chains:
        ready_at[c["id"]] = 0 if c["start"][0] in ("nib", "chan") else None
    running = []     # [chain_id, next_step]
    pending = [c["id"] for c in chains]
    out = []
    t = 0
    while pending or running:
        cand = [cid for cid in pending if ready_at[cid] is not None and ready_at[cid] <= t]
        cand.sort(key=lambda cid: (-by_id[cid]["prio"], chains.index(by_id[cid])))
        while len(running) < L and cand:
            cid = cand.pop(0)
            pending.remove(cid)
            running.append([cid, 0])
        if not running:
            raise RuntimeError("deadlock")
        issued = []
        for r in running:
            issued.append((r[0], r[1]))
            r[1] += 1
        out.append((t, issued))
        # exports become available next step
        for cid, k in issued:
            for c in chains:
                st = c["start"]
                if st[0] == "val" and st[1] == cid and st[2] == k:
                    ready_at[c["id"]] = t + 1
        running = [r for r in running if r[1] < len(by_id[r[0]]["steps"])]
        t += 1
    return out


def emit_body(kind, D, S, L):
    chains = cn_chains(D) if kind == "cn" else vn_chains(D)
    by_id = {c["id"]: c for c in chains}
    sched = schedule(chains, L)
    # column base of the last input: final-table slot added once, not per codeword
    lines = ["  const uint32_t lane4f = lane4 + fbase;"]
    u8_in = sorted({s[1] for c in chains for s in c["steps"]})
    for j in u8_in:
        for s in range(S):
            base = "lane4f" if j == D - 1 else "lane4"
            lines.append(f"  const uint32_t q{j}_{s} = colq(in[{j}], k0 + {s}, {base});")
    if kind == "vn":   # channel nibble as a row term: luc merges it with a column term in one v_lshl_or
        for s in range(S):
            lines.append(f"  const uint32_t c_{s} = nib(chw, k0 + {s});")

    def name(cid, k, s):
        return f"v_{cid}_{k}_{s}"

    def start_val(c, s):
        st = c["start"]
        if st[0] == "nib":
            return f"nib(in[{st[1]}], k0 + {s})"
        if st[0] == "val":
            return name(st[1], st[2], s)
        raise AssertionError

    for t, issued in sched:
        lines.append(f"  // step {t}: " + ", ".join(f"{cid}[{k}]" for cid, k in issued))
        for cid, k in issued:
            c = by_id[cid]
            op, j, sl, _ = c["steps"][k]
            for s in range(S):
                if op == "c":
                    expr = f"luc(c_{s}, q{j}_{s}, {sl})"
                else:
                    prev = start_val(c, s) if k == 0 else name(cid, k - 1, s)
                    expr = f"luc({prev}, q{j}_{s}, {sl})"
                lines.append(f"  const uint32_t {name(cid, k, s)} = {expr};")
        for cid, k in issued:
            c = by_id[cid]
            if k == len(c["steps"]) - 1:
                pk = name(cid, k, 0)
                for s in range(1, S):
                    pk = f"{pk} | ({name(cid, k, s)} << {4 * s})"
                lines.append(f"  o[{c['out']}] |= ({pk}) << (4 * k0);")
    return lines


def emit_body_cp(D, S, L):
    """The loop-form variable body of the degree whose composite table the launch staged (vn_group_cp<D>, degrees
    5..8): emit_body("vn", ..) with the chains of outputs 0 .. D-3 ending in one read of the composite's dword (lucw;
    column term colk, shared by those chains) whose nibble (cnib at shk's shift) is taken when the word is packed.
    Input D-2 then meets only the final table (on the Q chain), so like input D-1 it carries the table's run-time
    slot in its lane term and its lookups take no offset."""
    chains = vn_chains_composite(D)
    by_id = {c["id"]: c for c in chains}
    sched = schedule(chains, L)
    steps = [st for c in chains for st in c["steps"]]
    u8_in = sorted({st[1] for st in steps if st[0] != "k"})
    q_final = {j for j in u8_in if j == D - 1 or {st[2] for st in steps if st[1] == j and st[0] != "k"} == {"fbase"}}
    assert q_final == {D - 2, D - 1}
    lines = ["  const uint32_t lane4f = lane4 + fbase, lane4k = lane4 + kSuper;"]
    for j in u8_in:
        for s in range(S):
            lines.append(f"  const uint32_t q{j}_{s} = colq(in[{j}], k0 + {s}, {'lane4f' if j in q_final else 'lane4'});")
    for s in range(S):
        lines.append(f"  const uint32_t qk_{s} = colk(in[{D - 2}], in[{D - 1}], k0 + {s}, lane4k);")
        lines.append(f"  const uint32_t sh_{s} = shk(in[{D - 1}], k0 + {s});")
    for s in range(S):
        lines.append(f"  const uint32_t c_{s} = nib(chw, k0 + {s});")

    def name(cid, k, s):
        return f"v_{cid}_{k}_{s}"

    for t, issued in sched:
        lines.append(f"  // step {t}: " + ", ".join(f"{cid}[{k}]" for cid, k in issued))
        for cid, k in issued:
            c = by_id[cid]
            op, j, sl, _ = c["steps"][k]
            for s in range(S):
                if op == "c":
                    expr = f"luc(c_{s}, q{j}_{s}, {sl})"
                else:
                    st = c["start"]
                    assert k or st[0] == "val"
                    prev = name(cid, k - 1, s) if k else name(st[1], st[2], s)
                    expr = f"lucw({prev}, qk_{s})" if op == "k" else f"luc({prev}, q{j}_{s}, {'0u' if j in q_final else sl})"
                lines.append(f"  const uint32_t {name(cid, k, s)} = {expr};")
        for cid, k in issued:
            c = by_id[cid]
            if k == len(c["steps"]) - 1:
                def val(s):
                    return f"cnib({name(cid, k, s)}, sh_{s})" if c["steps"][k][0] == "k" else name(cid, k, s)
                pk = val(0)
                for s in range(1, S):
                    pk = f"{pk} | ({val(s)} << {4 * s})"
                lines.append(f"  o[{c['out']}] |= ({pk}) << (4 * k0);")
    return lines


def main():
    """args: S_cn L_cn [S_vn L_vn [S_vk L_vk]] (group size and chain lanes per kernel, for degrees <= 8; larger
    degrees use S = 2, L = 4 so the MAXD = 16 bodies keep their occupancy; S_vk L_vk: the variable pass's composite
    bodies, default 2 4)."""
    a = [int(x) for x in sys.argv[1:]] or [4, 2, 2, 4]
    Sc, Lc = a[0], a[1]
    Sv, Lv = (a[2], a[3]) if len(a) >= 4 else (Sc, Lc)
    Sk, Lk = (a[4], a[5]) if len(a) >= 6 else (2, 4)

    def cfg(S, L, D):
        return (S, L) if D <= 8 else (2, 4)
    print(f"// GENERATED by tools/gen_sched.py {' '.join(sys.argv[1:])} -- do not edit.")
    print(f"// Fold schedules of the IB fast path (degrees <= 8): CN groups of {Sc} codewords with up to {Lc}")
    print(f"// chains in flight, VN groups of {Sv} codewords with up to {Lv}; degrees > 8: 2 codewords, 4 chains.")
    print(f"__host__ __device__ constexpr int cn_sched_s(int D) {{ return D <= 8 ? {Sc} : 2; }}")
    print(f"__host__ __device__ constexpr int vn_sched_s(int D) {{ return D <= 8 ? {Sv} : 2; }}")
    print("template <int D> __device__ __forceinline__ void cn_group(uint32_t lane4, const uint32_t (&in)[D],")
    print("                                                         uint32_t fbase,")
    print("                                                         uint32_t (&o)[D], int k0);")
    print("template <int D> __device__ __forceinline__ void vn_group(uint32_t lane4, const uint32_t (&in)[D],")
    print("                                                         uint32_t chw, uint32_t fbase,")
    print("                                                         uint32_t (&o)[D], int k0);")
    for D in range(3, KMAXD + 1):
        print(f"template <> __device__ __forceinline__ void cn_group<{D}>(uint32_t lane4, const uint32_t (&in)[{D}],")
        print("                                                         uint32_t fbase,")
        print(f"                                                         uint32_t (&o)[{D}], int k0) {{")
        print("\n".join(emit_body("cn", D, *cfg(Sc, Lc, D))))
        print("}")
    for D in range(2, KMAXD + 1):
        print(f"template <> __device__ __forceinline__ void vn_group<{D}>(uint32_t lane4, const uint32_t (&in)[{D}],")
        print("                                                         uint32_t chw, uint32_t fbase,")
        print(f"                                                         uint32_t (&o)[{D}], int k0) {{")
        print("\n".join(emit_body("vn", D, *cfg(Sv, Lv, D))))
        print("}")
    # the variable pass's composite bodies (ib_vn_fast<8>, the degree whose composite table the launch staged)
    print(f"// Composite final step of the variable chains, degrees 5..8: groups of {Sk} codewords, {Lk} chains.")
    print(f"__host__ __device__ constexpr int vn_cp_sched_s() {{ return {Sk}; }}")
    print("template <int D> __device__ __forceinline__ void vn_group_cp(uint32_t lane4, const uint32_t (&in)[D],")
    print("                                                            uint32_t chw, uint32_t fbase,")
    print("                                                            uint32_t (&o)[D], int k0);")
    for D in range(5, 9):
        print(f"template <> __device__ __forceinline__ void vn_group_cp<{D}>(uint32_t lane4, const uint32_t (&in)[{D}],")
        print("                                                            uint32_t chw, uint32_t fbase,")
        print(f"                                                            uint32_t (&o)[{D}], int k0) {{")
        print("\n".join(emit_body_cp(D, Sk, Lk)))
        print("}")


# ----------------------------------------------------------------------------------------------------------------
# Unrolled bodies (csrc/ib_unrolled.inc, `python tools/gen_sched.py --unrolled [S_cn L_cn S_vn L_vn]`), degrees
# <= 8. The per-pass fast kernels of maximum degree 8 (and the fused kernel's light bodies) run a word's groups one
# after the other with the group's position a template argument: K0 = first codeword, ST = stride, codeword of
# sub-slot s = K0 + ST s. ST = 2 groups hold codewords of one parity, so a group needs one of each input word's two
# nibble spreads and one row/column word per first-level pair. Against the bodies above:
#   * output packing is one dependent chain acc = (t << 4k) | acc per word (pk<K>): 7 v_lshl_or_b32 per 8 nibbles,
#     none for nibble 0, no zeroing (the loop form: 10 per 8 and a v_mov_b32);
#   * a lookup whose two operands are raw input nibbles (chain start, or the channel) takes its whole address with
#     one v_perm_b32 (colb) from a word-level row/column byte (rowcol<P>: a shift and a v_bfi_b32 per word and
#     parity): no v_bfe_u32 and no v_lshl_or_b32 per codeword;
#   * an input whose column term meets only the final table at its run-time slot carries the slot in its lane term;
#   * emission order = issue order: every step ends with a scheduling barrier (step_fence), and a step is [column
#     terms first used here] [fold links of the chains that ended one step ago] [its lookups] [packing of the values
#     read one step ago], so the v_perm_b32 and the packing run in the shadow of LDS reads already issued. (Left to
#     itself the scheduler, at the register cap in a block this long, advances the chains diagonally and drains the
#     LDS queue 78 times per item instead of 41.)
# One line per chain step: the IBL_*<S> macros of ib_kernels.hip expand it over the S sub-slots (names n_0 .. n_{S-1}).
def emit_unrolled(kind, D, S, L, fold=False, comp=False):
    chains = (cn_chains_composite(D) if comp else cn_chains(D)) if kind == "cn" else vn_chains(D)
    by_id = {c["id"]: c for c in chains}
    sched = schedule(chains, L)
    assert S in (2, 4)

    def first_level(c, k):
        step = c["steps"][k]
        if step[0] == "c":
            return ("c", step[1])
        if k == 0 and c["start"][0] == "nib":
            return (c["start"][1], step[1])
        return None

    steps = [(c, k, st) for c in chains for k, st in enumerate(c["steps"])]
    fl = sorted({first_level(c, k) for c, k, _ in steps} - {None}, key=str)
    u8_in = sorted({st[1] for c, k, st in steps if not first_level(c, k) and st[0] != "k"})
    uses = {j: {st[2] for c, k, st in steps if st[1] == j and not first_level(c, k) and st[0] != "k"} for j in u8_in}
    q_final = {j for j in u8_in if j == D - 1 or uses[j] == {"fbase"}}
    lines = ["  const uint32_t lane4f = lane4 + fbase;"] + (["  const uint32_t lane4k = lane4 + kSuper;"] if comp else [])
    for a, j in fl:
        lines.append(f"  IBL_E(E{a}_{j}, {'chw' if a == 'c' else f'in[{a}]'}, in[{j}]);")
    defined, links, packs = set(), [], []

    def need(key):
        if key in defined:
            return []
        defined.add(key)
        if key == "k":   # the composite step's column term and nibble shift, shared by the D - 2 chains that end in it
            return [f"  IBL_QK{S}(qk, in[{D - 2}], in[{D - 1}], lane4k);", f"  IBL_SH{S}(sh, in[{D - 1}]);"]
        if isinstance(key, tuple):
            return [f"  IBL_QC{S}(qc{key[1]}, FC & {1 << key[1]}, ch{key[1]});"]
        return [f"  IBL_Q{S}(q{key}, in[{key}], {'lane4f' if key in q_final else 'lane4'});"]

    def flush(pre, look, done):
        nonlocal links, packs
        for a, cid, v in links:
            lines.extend(need(("qc", a)))
        lines.extend(pre)
        for a, cid, v in links:   # fold link: the degree-2 variable's update, F2(channel, this output)
            lines.append(f"  IBL_LINK{S}(f_{cid}, FC & {1 << a}, {v}, qc{a});")
        lines.extend(look)
        for out, v in packs:
            lines.append(f"  IBL_PKK{S}(o[{out}], {v[:-2]}, sh);" if v.endswith(":k") else f"  IBL_PK{S}(o[{out}], {v});")
        packs = [(by_id[cid]["out"], f"f_{cid}") for a, cid, v in links] + [d for d in done if d[0] is not None]
        links = [(d[1], d[2], d[3]) for d in done if d[0] is None]
        lines.append("  step_fence();")

    for t, issued in sched:
        pre, look, done = [], [], []
        for cid, k in issued:
            c = by_id[cid]
            op, j, sl, _ = c["steps"][k]
            f1 = first_level(c, k)
            name = f"v_{cid}_{k}"
            if op == "k":   # raw dword of the composite; its nibble is taken when the word is packed
                pre.extend(need("k"))
                st = c["start"]
                look.append(f"  IBL_LUK{S}({name}, {f'v_{cid}_{k - 1}' if k else f'v_{st[1]}_{st[2]}'}, qk);")
                assert k == len(c["steps"]) - 1 and (k or st[0] == "val")
                done.append((c["out"], name + ":k"))
                continue
            if f1:
                final = sl == "fbase" or j == D - 1
                look.append(f"  IBL_LU1{S}({name}, E{f1[0]}_{f1[1]}, {'lane4f, 0u' if final else 'lane4, ' + sl});")
            else:
                pre.extend(need(j))
                st = c["start"]
                prev = f"v_{cid}_{k - 1}" if k else f"v_{st[1]}_{st[2]}"
                assert k or st[0] == "val"
                look.append(f"  IBL_LUC{S}({name}, {prev}, q{j}, {'0u' if j in q_final else sl});")
            if k == len(c["steps"]) - 1:
                a = c["out"] - (D - 2)
                done.append((None, a, cid, name) if fold and a >= 0 else (c["out"], name))
        flush(pre, look, done)
    while links or packs:
        flush([], [], [])
    return lines


def main_unrolled(a):
    Sc, Lc, Sv, Lv = (a or [4, 2, 2, 4])[:4]   # (S_vk L_vk, the variable pass's composite loop bodies: ib_sched.inc only)
    print(f"// GENERATED by tools/gen_sched.py {' '.join(['--unrolled', *map(str, a)])} -- do not edit.")
    print(f"// Unrolled fold schedules of the IB fast path, degrees <= 8 (see tools/gen_sched.py): CN groups of {Sc}")
    print(f"// codewords, {Lc} chains; VN groups of {Sv}, {Lv} chains. K0 = first codeword, ST = stride of the group.")
    print(f"static_assert(cn_sched_s(8) == {Sc} && vn_sched_s(8) == {Sv},")
    print("              \"the unrolled bodies were generated for another schedule (IBL_UNROLLED_FILE)\");")
    cargs = "uint32_t lane4, const uint32_t (&in)[D], uint32_t fbase"
    # (the plain check bodies are the folding ones at FC = 0: cn_group_ct in ib_kernels.hip)
    # The variable bodies stop at degree 4, the fused kernel's light bodies: the per-pass variable kernel keeps the
    # loop bodies (unrolled it issued 12 % fewer VALU per lookup and was no faster).
    # cn_group_fold_cp: the form of the one check degree whose composite table is staged (degrees 5..8; issue order
    # as above, the composite step's nibble select runs with the packing, one step after its read)
    for kind, lo, hi, fold, comp in (("cn", 3, 8, True, False), ("cn", 5, 8, True, True), ("vn", 2, 4, False, False)):
        fn = f"{kind}_group{'_fold' if fold else ''}_{'cp' if comp else 'ct'}"
        extra = (", uint32_t lane4c, uint32_t ch0, uint32_t ch1" if fold else "") + (", uint32_t chw" if kind == "vn" else "")
        print(f"template <int D, {'int FC, ' if fold else ''}int K0, int ST{', bool LS' if comp else ''}> __device__ __forceinline__ void {fn}({cargs}{extra},")
        print("    uint32_t (&o)[D]) {")
        print(f"  static_assert(D >= {lo} && D <= {hi} && K0 >= 0 && (ST == 1 || ST == 2), \"unrolled bodies: degrees {lo}..{hi}\");")
        for D in range(lo, hi + 1):
            print(f"  if constexpr (D == {D}) {{")
            print("\n".join("  " + l for l in emit_unrolled(kind, D, Sc if kind == "cn" else Sv, Lc if kind == "cn" else Lv, fold, comp)))
            print("  }")
        print("}")


if __name__ == "__main__":
    if sys.argv[1:2] == ["--unrolled"]:
        main_unrolled([int(x) for x in sys.argv[2:]])
    else:
        main()
