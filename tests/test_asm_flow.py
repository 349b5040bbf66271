"""tests/asm_flow.py against known answers -- no GPU needed.

Small hand-written kernels, a dozen lines each, written for this test (not cut from the generators).  For every rule of passes A, B and
C: one kernel that must produce exactly that finding (and at the named instruction), and its repaired twin, which must produce none."""
import pytest

import asm_flow

PRE = """
s_load_dwordx4 s[8:11], s[0:1], 0x0
s_load_dwordx2 s[4:5], s[0:1], 0x10
s_waitcnt lgkmcnt(0)
"""                                             # s[8:11]: a buffer descriptor; s4, s5: values nothing is known about


def kernel(body, name="k", vgpr=32, accum=None, sgpr=32, lds=4096, end="s_endpgm"):
    lines = [l.strip() for l in (PRE + body + "\n" + end).strip().split("\n") if l.strip()]
    text = "\n".join(l if l.endswith(":") else "\t" + l for l in lines)
    return f"""\t.text
{name}:
{text}
.Lfend_{name}:
\t.amdhsa_kernel {name}
\t\t.amdhsa_group_segment_fixed_size {lds}
\t\t.amdhsa_user_sgpr_count 2
\t\t.amdhsa_user_sgpr_kernarg_segment_ptr 1
\t\t.amdhsa_system_sgpr_workgroup_id_x 1
\t\t.amdhsa_system_vgpr_workitem_id 0
\t\t.amdhsa_next_free_vgpr {vgpr}
\t\t.amdhsa_next_free_sgpr {sgpr}
\t\t.amdhsa_accum_offset {vgpr if accum is None else accum}
\t.end_amdhsa_kernel
"""


def findings(body, **kw):
    reports = asm_flow.check(kernel(body, **kw))
    assert len(reports) == 1 and reports[0].name == "k"
    return reports[0].findings


def zero(*regs):
    return "\n".join(f"v_mov_b32 v{r}, 0" for r in regs)


LOOP_TAIL = """
s_add_u32 s6, s6, 1
s_cmp_lt_u32 s6, s5
s_cbranch_scc1 .Lloop
"""


def counter_kernel(late):
    """Chunk loop inside a tile loop; the next chunk's load is issued a trip ahead, two stores follow a tile's last chunk, and chunk 0
    of every tile but the first waits with `late` (two stores are younger than its load) instead of 0."""
    return f"""
        {zero(8, 10, 11)}
        s_mov_b32 s6, 0
        s_mov_b32 s7, 1
        global_load_dwordx2 v[2:3], v0, s[0:1]
        .Lloop:
        s_cmp_eq_u32 s6, 0
        s_cselect_b32 s12, 1, 0
        s_cmp_eq_u32 s7, 1
        s_cselect_b32 s12, 0, s12
        s_cmp_eq_u32 s12, 1
        s_cbranch_scc1 .Llate
        s_waitcnt vmcnt(0)
        .Ljoin:
        v_add_u32 v8, v8, v2
        global_load_dwordx2 v[2:3], v0, s[0:1] offset:8
        s_mov_b32 s7, 0
        {LOOP_TAIL}
        global_store_dwordx2 v0, v[10:11], s[0:1] offset:64
        global_store_dwordx2 v0, v[10:11], s[0:1] offset:72
        s_mov_b32 s6, 0
        s_cmp_eq_u32 s4, 0
        s_cbranch_scc0 .Lloop
        s_branch .Lend
        .Llate:
        s_waitcnt vmcnt({late})
        s_branch .Ljoin
        .Lend:
        s_waitcnt vmcnt(0)"""



def back_edge_kernel(pad):
    """A VALU writes s7 at the bottom of a loop; the load that takes s7 sits in the FALL-THROUGH arm of a branch at the top, four wait
    states behind the write by way of the back edge (five with `pad`)."""
    return f"""
        s_mov_b32 s7, 0
        .Lloop:
        s_lshr_b32 s13, s4, 1
        s_cmp_eq_u32 s13, 0
        s_cbranch_scc1 .Lother
        buffer_load_dwordx2 v[4:5], v0, s[8:11], s7 offen
        s_branch .Ljoin
        .Lother:
        s_nop 0
        .Ljoin:
        s_waitcnt vmcnt(0)
        s_cmp_lt_u32 s4, s5
        v_readfirstlane_b32 s7, v0{pad}
        s_cbranch_scc0 .Lloop"""


# name -> (rule, the instruction the finding must name, broken kernel, repaired kernel)
CASES = {
    # ---- pass A ----
    "vmem load read one wait too early": ("read-pending", "v_add_u32 v6, v4, v2", """
        global_load_dwordx2 v[2:3], v0, s[0:1]
        global_load_dwordx2 v[4:5], v0, s[0:1] offset:8
        s_waitcnt vmcnt(1)
        v_add_u32 v6, v4, v2
        s_waitcnt vmcnt(0)""", """
        global_load_dwordx2 v[2:3], v0, s[0:1]
        global_load_dwordx2 v[4:5], v0, s[0:1] offset:8
        s_waitcnt vmcnt(0)
        v_add_u32 v6, v4, v2"""),
    # two-stage pipeline: the load at the bottom of a trip is consumed at the top of the next one, across the back edge
    "pipelined loop, load consumed in the next trip": ("read-pending", "v_add_u32 v8, v8, v2", f"""
        v_mov_b32 v8, 0
        s_mov_b32 s6, 0
        global_load_dwordx2 v[2:3], v0, s[0:1]
        .Lloop:
        global_load_dwordx2 v[4:5], v0, s[0:1] offset:8
        s_waitcnt vmcnt(2)
        v_add_u32 v8, v8, v2
        global_load_dwordx2 v[2:3], v0, s[0:1] offset:16
        s_waitcnt vmcnt(1)
        v_add_u32 v8, v8, v4
        {LOOP_TAIL}
        s_waitcnt vmcnt(0)""", f"""
        v_mov_b32 v8, 0
        s_mov_b32 s6, 0
        global_load_dwordx2 v[2:3], v0, s[0:1]
        .Lloop:
        global_load_dwordx2 v[4:5], v0, s[0:1] offset:8
        s_waitcnt vmcnt(1)
        v_add_u32 v8, v8, v2
        global_load_dwordx2 v[2:3], v0, s[0:1] offset:16
        s_waitcnt vmcnt(1)
        v_add_u32 v8, v8, v4
        {LOOP_TAIL}
        s_waitcnt vmcnt(0)"""),
    "join, the load pending on one arm only": ("read-pending", "v_add_u32 v6, v2, v2", f"""
        {zero(2, 3)}
        s_cmp_eq_u32 s4, 0
        s_cbranch_scc1 .Lskip
        global_load_dwordx2 v[2:3], v0, s[0:1]
        .Lskip:
        v_add_u32 v6, v2, v2
        s_waitcnt vmcnt(0)""", f"""
        {zero(2, 3)}
        s_cmp_eq_u32 s4, 0
        s_cbranch_scc1 .Lskip
        global_load_dwordx2 v[2:3], v0, s[0:1]
        .Lskip:
        s_waitcnt vmcnt(0)
        v_add_u32 v6, v2, v2"""),
    # SMEM returns out of order: lgkmcnt(1) says one of the two is back, not which
    "s_load behind lgkmcnt(1)": ("read-pending", "s_add_u32 s7, s6, 1", """
        s_load_dword s6, s[0:1], 0x20
        ds_read_b128 v[4:7], v0
        s_waitcnt lgkmcnt(1)
        s_add_u32 s7, s6, 1
        s_waitcnt lgkmcnt(0)""", """
        s_load_dword s6, s[0:1], 0x20
        ds_read_b128 v[4:7], v0
        s_waitcnt lgkmcnt(0)
        s_add_u32 s7, s6, 1"""),
    # an LDS-DMA has no register destination and still counts on vmcnt: with it in between, vmcnt(1) covers the load, vmcnt(2) does not
    "LDS-DMA between a load and its wait": ("read-pending", "v_add_u32 v6, v2, v3", """
        global_load_dwordx2 v[2:3], v0, s[0:1]
        s_mov_b32 m0, 0
        s_nop 0
        buffer_load_dwordx4 v0, s[8:11], 0 offen lds
        s_waitcnt vmcnt(2)
        v_add_u32 v6, v2, v3
        s_waitcnt vmcnt(0)""", """
        global_load_dwordx2 v[2:3], v0, s[0:1]
        s_mov_b32 m0, 0
        s_nop 0
        buffer_load_dwordx4 v0, s[8:11], 0 offen lds
        s_waitcnt vmcnt(1)
        v_add_u32 v6, v2, v3
        s_waitcnt vmcnt(0)"""),
    "global_load_lds counts as well": ("read-pending", "v_add_u32 v6, v2, v3", f"""
        {zero(20, 21)}
        global_load_dwordx2 v[2:3], v0, s[0:1]
        s_mov_b32 m0, 0
        s_nop 0
        global_load_lds_dwordx4 v[20:21], off
        s_waitcnt vmcnt(2)
        v_add_u32 v6, v2, v3
        s_waitcnt vmcnt(0)""", f"""
        {zero(20, 21)}
        global_load_dwordx2 v[2:3], v0, s[0:1]
        s_mov_b32 m0, 0
        s_nop 0
        global_load_lds_dwordx4 v[20:21], off
        s_waitcnt vmcnt(1)
        v_add_u32 v6, v2, v3
        s_waitcnt vmcnt(0)"""),
    # 70 operations behind the first load: its count saturates at 63 and vmcnt(63) retires it; the youngest stays pending
    "more than 63 operations behind a load": ("read-pending", "v_add_u32 v6, v10, v10", """
        global_load_dwordx2 v[2:3], v0, s[0:1]
        """ + "\n".join(f"global_load_dwordx2 v[{10 + 2 * (i % 8)}:{11 + 2 * (i % 8)}], v0, s[0:1] offset:{8 * i}" for i in range(70)) + """
        s_waitcnt vmcnt(63)
        v_add_u32 v6, v10, v10
        s_waitcnt vmcnt(0)""", """
        global_load_dwordx2 v[2:3], v0, s[0:1]
        """ + "\n".join(f"global_load_dwordx2 v[{10 + 2 * (i % 8)}:{11 + 2 * (i % 8)}], v0, s[0:1] offset:{8 * i}" for i in range(70)) + """
        s_waitcnt vmcnt(63)
        v_add_u32 v6, v2, v3
        s_waitcnt vmcnt(0)"""),
    "lds reads return in order, ds_bpermute counts": ("read-pending", "v_add_u32 v20, v8, v8", f"""
        {zero(9)}
        ds_read_b128 v[4:7], v0
        ds_bpermute_b32 v8, v0, v9
        s_waitcnt lgkmcnt(1)
        v_add_u32 v20, v8, v8
        s_waitcnt lgkmcnt(0)""", f"""
        {zero(9)}
        ds_read_b128 v[4:7], v0
        ds_bpermute_b32 v8, v0, v9
        s_waitcnt lgkmcnt(1)
        v_add_u32 v20, v4, v4
        s_waitcnt lgkmcnt(0)"""),
    "lds write between a read and its wait counts": ("read-pending", "v_add_u32 v20, v4, v4", f"""
        {zero(8, 9)}
        ds_read_b128 v[4:7], v0
        ds_write_b64 v0, v[8:9] offset:64
        s_waitcnt lgkmcnt(2)
        v_add_u32 v20, v4, v4
        s_waitcnt lgkmcnt(0)""", f"""
        {zero(8, 9)}
        ds_read_b128 v[4:7], v0
        ds_write_b64 v0, v[8:9] offset:64
        s_waitcnt lgkmcnt(1)
        v_add_u32 v20, v4, v4
        s_waitcnt lgkmcnt(0)"""),
    "the address of a pending load's destination": ("read-pending", "global_load_dwordx2 v[4:5], v2, s[0:1]", """
        global_load_dwordx2 v[2:3], v0, s[0:1]
        global_load_dwordx2 v[4:5], v2, s[0:1]
        s_waitcnt vmcnt(0)""", """
        global_load_dwordx2 v[2:3], v0, s[0:1]
        s_waitcnt vmcnt(0)
        global_load_dwordx2 v[4:5], v2, s[0:1]
        s_waitcnt vmcnt(0)"""),
    "VALU write of a register a load is filling": ("write-pending", "v_mov_b32 v2, 0", """
        global_load_dwordx2 v[2:3], v0, s[0:1]
        v_mov_b32 v2, 0
        s_waitcnt vmcnt(0)""", """
        global_load_dwordx2 v[2:3], v0, s[0:1]
        s_waitcnt vmcnt(0)
        v_mov_b32 v2, 0"""),
    # a load on the SAME counter may overwrite (in order); one on the other counter may not
    "lds read into a register a vmem load is filling": ("write-pending", "ds_read_b128 v[2:5], v0", """
        global_load_dwordx2 v[2:3], v0, s[0:1]
        ds_read_b128 v[2:5], v0
        s_waitcnt vmcnt(0)
        s_waitcnt lgkmcnt(0)""", """
        global_load_dwordx2 v[2:3], v0, s[0:1]
        global_load_dwordx4 v[2:5], v0, s[0:1]
        s_waitcnt vmcnt(0)"""),
    "store in flight at s_endpgm": ("end-undrained", "s_endpgm", f"""
        {zero(2, 3)}
        global_store_dwordx2 v0, v[2:3], s[0:1]""", f"""
        {zero(2, 3)}
        global_store_dwordx2 v0, v[2:3], s[0:1]
        s_waitcnt vmcnt(0)"""),
    "LDS-DMA in flight at s_endpgm on one path": ("end-undrained", "s_endpgm", """
        s_cmp_eq_u32 s4, 0
        s_cbranch_scc1 .Lend
        s_mov_b32 m0, 0
        s_nop 0
        buffer_load_dwordx4 v0, s[8:11], 0 offen lds
        s_waitcnt vmcnt(1)
        .Lend:""", """
        s_cmp_eq_u32 s4, 0
        s_cbranch_scc1 .Lend
        s_mov_b32 m0, 0
        s_nop 0
        buffer_load_dwordx4 v0, s[8:11], 0 offen lds
        .Lend:
        s_waitcnt vmcnt(0)"""),
    # ---- scalar flags: the wait of one arm belongs to the loads of that arm's paths ----
    # A flag set behind two stores selects the looser wait; merging all paths into one state per block would hold vmcnt(2) against the
    # path without stores.
    "flag-selected wait, the store path's count too loose": ("read-pending", "v_add_u32 v8, v8, v2", f"""
        {zero(8, 10, 11)}
        s_mov_b32 s6, 0
        s_mov_b32 s7, 0
        .Lloop:
        global_load_dwordx2 v[2:3], v0, s[0:1]
        s_cmp_eq_u32 s4, 0
        s_cbranch_scc1 .Lnostore
        global_store_dwordx2 v0, v[10:11], s[0:1] offset:64
        global_store_dwordx2 v0, v[10:11], s[0:1] offset:72
        s_mov_b32 s7, 1
        .Lnostore:
        s_cmp_eq_u32 s7, 1
        s_cbranch_scc1 .Llate
        s_waitcnt vmcnt(0)
        s_branch .Ljoin
        .Llate:
        s_waitcnt vmcnt(3)
        .Ljoin:
        v_add_u32 v8, v8, v2
        s_mov_b32 s7, 0
        {LOOP_TAIL}
        s_waitcnt vmcnt(0)""", f"""
        {zero(8, 10, 11)}
        s_mov_b32 s6, 0
        s_mov_b32 s7, 0
        .Lloop:
        global_load_dwordx2 v[2:3], v0, s[0:1]
        s_cmp_eq_u32 s4, 0
        s_cbranch_scc1 .Lnostore
        global_store_dwordx2 v0, v[10:11], s[0:1] offset:64
        global_store_dwordx2 v0, v[10:11], s[0:1] offset:72
        s_mov_b32 s7, 1
        .Lnostore:
        s_cmp_eq_u32 s7, 1
        s_cbranch_scc1 .Llate
        s_waitcnt vmcnt(0)
        s_branch .Ljoin
        .Llate:
        s_waitcnt vmcnt(2)
        .Ljoin:
        v_add_u32 v8, v8, v2
        s_mov_b32 s7, 0
        {LOOP_TAIL}
        s_waitcnt vmcnt(0)"""),
    # "chunk 0 of a tile that is not the first": a counter compared with 0, reset behind the stores.  A counter known as "not 0" must
    # stay so after + 1, in either operand order, or chunk 1 takes chunk 0's arm.
    "counter-selected wait behind an epilogue": ("read-pending", "v_add_u32 v8, v8, v2", counter_kernel(3), counter_kernel(2)),
    # ---- pass B ----
    "read before write on one arm": ("read-before-write", "v_add_u32 v5, v4, v0", """
        s_cmp_eq_u32 s4, 0
        s_cbranch_scc1 .Lelse
        v_mov_b32 v4, 1
        .Lelse:
        v_add_u32 v5, v4, v0""", """
        v_mov_b32 v4, 0
        s_cmp_eq_u32 s4, 0
        s_cbranch_scc1 .Lelse
        v_mov_b32 v4, 1
        .Lelse:
        v_add_u32 v5, v4, v0"""),
    "read before write, half of a pair": ("read-before-write", "global_store_dwordx2 v0, v[4:5], s[0:1]", """
        v_mov_b32 v4, 1
        global_store_dwordx2 v0, v[4:5], s[0:1]
        s_waitcnt vmcnt(0)""", """
        v_mov_b32 v4, 1
        v_mov_b32 v5, 1
        global_store_dwordx2 v0, v[4:5], s[0:1]
        s_waitcnt vmcnt(0)"""),
    # a write under a partial exec counts as a write
    "written under a partial exec on one arm only": ("read-before-write", "v_add_u32 v5, v4, v0", """
        s_cmp_eq_u32 s4, 0
        s_cbranch_scc1 .Lelse
        v_cmp_gt_u32 vcc, 8, v0
        s_and_saveexec_b64 s[6:7], vcc
        v_mov_b32 v4, 1
        s_mov_b64 exec, s[6:7]
        .Lelse:
        v_add_u32 v5, v4, v0""", """
        s_cmp_eq_u32 s4, 0
        s_cbranch_scc1 .Lelse
        v_cmp_gt_u32 vcc, 8, v0
        s_and_saveexec_b64 s[6:7], vcc
        v_mov_b32 v4, 1
        s_mov_b64 exec, s[6:7]
        s_branch .Luse
        .Lelse:
        v_mov_b32 v4, 2
        .Luse:
        v_add_u32 v5, v4, v0"""),
    "an SGPR the descriptor does not initialise": ("read-before-write", "s_add_u32 s6, s3, 1", """
        s_add_u32 s6, s3, 1""", """
        s_add_u32 s6, s2, 1"""),
    "scc read with nothing setting it": ("read-before-write", "s_cselect_b32 s6, 1, 0", """
        s_cselect_b32 s6, 1, 0""", """
        s_cmp_eq_u32 s4, 0
        s_cselect_b32 s6, 1, 0"""),
    "m0 never written ahead of an LDS-DMA": ("read-before-write", "buffer_load_dwordx4 v0, s[8:11], 0 offen lds", """
        buffer_load_dwordx4 v0, s[8:11], 0 offen lds
        s_waitcnt vmcnt(0)""", """
        s_mov_b32 m0, 0
        s_nop 0
        buffer_load_dwordx4 v0, s[8:11], 0 offen lds
        s_waitcnt vmcnt(0)"""),
    "vgpr one past the budget": ("vgpr-budget", "v_mov_b32 v32, 0", "v_mov_b32 v32, 0", "v_mov_b32 v31, 0"),
    "sgpr one past the budget": ("sgpr-budget", "s_mov_b32 s32, 0", "s_mov_b32 s32, 0", "s_mov_b32 s31, 0"),
    # ---- pass C ----
    "MFMA result read by a VALU too early": ("mfma-result", "v_mov_b32 v20, v4", f"""
        {zero(*range(4, 16))}
        v_mfma_f32_16x16x32_bf16 v[4:7], v[8:11], v[12:15], v[4:7]
        s_nop 14
        v_mov_b32 v20, v4""", f"""
        {zero(*range(4, 16))}
        v_mfma_f32_16x16x32_bf16 v[4:7], v[8:11], v[12:15], v[4:7]
        s_nop 15
        v_mov_b32 v20, v4"""),
    # the accumulate chain of one kind needs nothing; a store of the result does
    "MFMA result as store data": ("mfma-result", "global_store_dwordx4 v0, v[4:7], s[0:1]", f"""
        {zero(*range(4, 16))}
        v_mfma_f32_16x16x32_bf16 v[4:7], v[8:11], v[12:15], v[4:7]
        v_mfma_f32_16x16x32_bf16 v[4:7], v[8:11], v[12:15], v[4:7]
        s_nop 14
        global_store_dwordx4 v0, v[4:7], s[0:1]
        s_waitcnt vmcnt(0)""", f"""
        {zero(*range(4, 16))}
        v_mfma_f32_16x16x32_bf16 v[4:7], v[8:11], v[12:15], v[4:7]
        v_mfma_f32_16x16x32_bf16 v[4:7], v[8:11], v[12:15], v[4:7]
        s_nop 15
        global_store_dwordx4 v0, v[4:7], s[0:1]
        s_waitcnt vmcnt(0)"""),
    "transcendental result used by the next instruction": ("trans-result", "v_mul_f32 v5, v4, v4", """
        v_exp_f32 v4, v0
        v_mul_f32 v5, v4, v4""", """
        v_exp_f32 v4, v0
        v_mov_b32 v6, 0
        v_mul_f32 v5, v4, v4"""),
    "m0 written right ahead of an LDS-DMA": ("m0-dma", "buffer_load_dwordx4 v0, s[8:11], 0 offen lds", """
        s_mov_b32 m0, 0
        buffer_load_dwordx4 v0, s[8:11], 0 offen lds
        s_waitcnt vmcnt(0)""", """
        s_mov_b32 m0, 0
        s_nop 0
        buffer_load_dwordx4 v0, s[8:11], 0 offen lds
        s_waitcnt vmcnt(0)"""),
    # the hazard is followed into the next block, and at a join the younger write decides
    "m0 written at the end of one arm into an LDS-DMA": ("m0-dma", "global_load_lds_dwordx4 v[20:21], off", f"""
        {zero(20, 21)}
        s_cmp_eq_u32 s4, 0
        s_cbranch_scc1 .Lother
        s_add_u32 m0, s4, 64
        .Ldma:
        global_load_lds_dwordx4 v[20:21], off
        s_branch .Lend
        .Lother:
        s_mov_b32 m0, 0
        s_nop 0
        s_branch .Ldma
        .Lend:
        s_waitcnt vmcnt(0)""", f"""
        {zero(20, 21)}
        s_cmp_eq_u32 s4, 0
        s_cbranch_scc1 .Lother
        s_add_u32 m0, s4, 64
        s_nop 0
        .Ldma:
        global_load_lds_dwordx4 v[20:21], off
        s_branch .Lend
        .Lother:
        s_mov_b32 m0, 0
        s_nop 0
        s_branch .Ldma
        .Lend:
        s_waitcnt vmcnt(0)"""),
    "VALU write one state ahead of v_readfirstlane": ("valu-readfirstlane", "v_readfirstlane_b32 s6, v4", """
        v_lshrrev_b32 v4, 6, v0
        s_nop 0
        v_readfirstlane_b32 s6, v4""", """
        v_lshrrev_b32 v4, 6, v0
        s_nop 1
        v_readfirstlane_b32 s6, v4"""),
    "VALU write one state ahead of a permlane swap": ("valu-permlane", "v_permlane32_swap_b32 v4, v5", """
        v_mov_b32 v4, 1
        v_mov_b32 v5, 2
        s_nop 0
        v_permlane32_swap_b32 v4, v5""", """
        v_mov_b32 v4, 1
        v_mov_b32 v5, 2
        s_nop 1
        v_permlane32_swap_b32 v4, v5"""),
    "VALU-written SGPR four states ahead of a VMEM": ("valu-sgpr-vmem", "buffer_load_dwordx2 v[4:5], v0, s[8:11], s6 offen", """
        v_readfirstlane_b32 s6, v0
        s_nop 3
        buffer_load_dwordx2 v[4:5], v0, s[8:11], s6 offen
        s_waitcnt vmcnt(0)""", """
        v_readfirstlane_b32 s6, v0
        s_nop 4
        buffer_load_dwordx2 v[4:5], v0, s[8:11], s6 offen
        s_waitcnt vmcnt(0)"""),
    "v_cmp mask as the base of a global load": ("valu-sgpr-vmem", "global_load_dwordx2 v[4:5], v0, s[6:7]", """
        v_cmp_gt_u32 s[6:7], 8, v0
        s_nop 0
        global_load_dwordx2 v[4:5], v0, s[6:7]
        s_waitcnt vmcnt(0)""", """
        v_cmp_gt_u32 s[6:7], 8, v0
        s_nop 4
        global_load_dwordx2 v[4:5], v0, s[6:7]
        s_waitcnt vmcnt(0)"""),
    # the state handed to the two successors of a branch must be two objects: with shared inner tables the younger write that arrives
    # by the back edge reached the taken arm only, and the load in the fall-through arm went unreported
    "hazard across the back edge into the fall-through arm": ("valu-sgpr-vmem", "buffer_load_dwordx2 v[4:5], v0, s[8:11], s7 offen",
                                                              back_edge_kernel(""), back_edge_kernel("\n        s_nop 0")),
    "data of a 16-byte store rewritten behind it": ("store16-data", "v_mov_b32 v5, 1", f"""
        {zero(4, 5, 6, 7)}
        s_nop 1
        global_store_dwordx4 v0, v[4:7], s[0:1]
        s_nop 0
        v_mov_b32 v5, 1
        s_waitcnt vmcnt(0)""", f"""
        {zero(4, 5, 6, 7)}
        s_nop 1
        global_store_dwordx4 v0, v[4:7], s[0:1]
        s_nop 1
        v_mov_b32 v5, 1
        s_waitcnt vmcnt(0)"""),
    # an 8-byte store needs nothing
    "data of a 16-byte buffer store rewritten behind it": ("store16-data", "v_exp_f32 v4, v0", f"""
        {zero(4, 5, 6, 7)}
        buffer_store_dwordx4 v[4:7], v0, s[8:11], 0 offen
        v_exp_f32 v4, v0
        s_waitcnt vmcnt(0)""", f"""
        {zero(4, 5, 6, 7)}
        buffer_store_dwordx2 v[4:5], v0, s[8:11], 0 offen
        v_exp_f32 v4, v0
        s_waitcnt vmcnt(0)"""),
    # ---- the table ----
    "a source modifier the operand pattern does not read": ("unclassified", "v_add_f32_e64 v4, v0, -v2", f"""
        {zero(2)}
        v_add_f32_e64 v4, v0, -v2""", f"""
        {zero(2)}
        v_add_f32_e64 v4, v0, v2"""),
    "a mnemonic that is not in the table": ("unclassified", "v_fma_f32 v4, v0, v0, v0", "v_fma_f32 v4, v0, v0, v0", "v_add3_u32 v4, v0, v0, v0"),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_snippet_and_its_repaired_twin(name):
    rule, text, bad, good = CASES[name]
    got = findings(bad)
    assert [f.rule for f in got] == [rule], [tuple(f) for f in got]
    assert got[0].text == text and got[0].kernel == "k"
    assert findings(good) == []


def test_agpr_budget_and_accum_offset():
    body = zero(4, 5, 6, 7) + "\nv_mfma_f32_16x16x32_bf16 a[{0}:{1}], v[4:7], v[4:7], 0"
    assert findings(body.format(0, 3), vgpr=12, accum=8) == []
    got = findings(body.format(1, 4), vgpr=12, accum=8)                   # a4 of 12 - 8 = 4 accumulator registers
    assert [f.rule for f in got] == ["agpr-budget"] and "a4" in got[0].detail
    got = findings("v_mov_b32 v8, 0", vgpr=12, accum=8)                   # the VGPRs end at accum_offset, not at next_free_vgpr
    assert [f.rule for f in got] == ["vgpr-budget"]


def test_static_lds_offsets():
    assert findings("ds_read_b128 v[4:7], v0 offset:4080\ns_waitcnt lgkmcnt(0)") == []
    got = findings("ds_read_b128 v[4:7], v0 offset:4096\ns_waitcnt lgkmcnt(0)")
    assert [f.rule for f in got] == ["lds-offset"]
    got = findings(zero(4, 5) + "\nds_write_b64 v0, v[4:5] offset:8192\ns_waitcnt lgkmcnt(0)")
    assert [f.rule for f in got] == ["lds-offset"]
    assert [f.rule for f in findings("s_mov_b32 m0, 4096")] == ["lds-offset"]
    assert [f.rule for f in findings("s_add_u32 m0, s4, 0x1000")] == ["lds-offset"]
    assert findings("s_add_u32 m0, s4, 0xfff") == []


def test_a_load_never_waited_for_in_a_loop_saturates_and_ends():
    """Without saturation (and the worst-case join) the count of the first load would grow with every trip."""
    body = f"s_mov_b32 s6, 0\nglobal_load_dwordx2 v[2:3], v0, s[0:1]\n.Lloop:\nglobal_load_dwordx2 v[4:5], v0, s[0:1]\n{LOOP_TAIL}\ns_waitcnt vmcnt(0)"
    assert findings(body) == []
    k = asm_flow.split_kernels(kernel(body))[0]
    blocks, succs, _ = asm_flow.expand_cfg(k)
    states = asm_flow._pass_a(k, blocks, succs, asm_flow.KernelReport("k"), lambda *a: None)
    counts = [st[0][2] for st in states if st is not None and 2 in st[0]]
    assert counts and max(counts) <= asm_flow.VMCNT_MAX


def test_counts_and_parsing():
    rep = asm_flow.check(kernel(CASES["LDS-DMA between a load and its wait"][3]))[0]
    assert rep.loads == 1 + 2 and rep.waits == 2 + 1                     # the prologue's two s_loads and its wait included
    assert rep.sites["m0-dma"] == 1
    x = asm_flow.parse_instruction("buffer_load_dwordx4 v[1:4], v5, s[8:11], s3 offen offset:1024")
    assert x.cls == asm_flow.VLOAD and x.writes == (1, 2, 3, 4) and x.mods == ("offen", "offset:1024")
    assert set(x.reads) == {5, asm_flow.S0 + 3} | {asm_flow.S0 + i for i in range(8, 12)}
    x = asm_flow.parse_instruction("buffer_load_dwordx4 v5, s[8:11], 0 offen lds")
    assert x.cls == asm_flow.LDSDMA and x.writes == () and asm_flow.M0 in x.reads and 5 in x.reads
    x = asm_flow.parse_instruction("v_cvt_pk_f32_fp8_sdwa v[2:3], v9 src0_sel:WORD_1")
    assert x.writes == (2, 3) and x.reads == (9,)
    x = asm_flow.parse_instruction("v_addc_co_u32 v1, vcc, 0, v2, vcc")
    assert set(x.writes) == {1, asm_flow.VCC, asm_flow.VCC + 1} and set(x.reads) == {2, asm_flow.VCC, asm_flow.VCC + 1}
    x = asm_flow.parse_instruction("v_permlane16_swap_b32 v4, v7")
    assert set(x.writes) == {4, 7} == set(x.reads)
    x = asm_flow.parse_instruction("global_store_dwordx4 v9, v[4:7], s[2:3] offset:64")
    assert x.data == (4, 5, 6, 7) and x.writes == ()
    x = asm_flow.parse_instruction("s_waitcnt vmcnt(3) lgkmcnt(1)")
    assert x.imm == {"vmcnt": 3, "lgkmcnt": 1}
    assert len(asm_flow.MNEMONICS) == 101                                 # what the four generators emit today


def test_two_kernels_in_one_file_are_told_apart():
    text = kernel("v_mov_b32 v32, 0", name="first") + kernel("v_mov_b32 v31, 0", name="second")
    reps = asm_flow.check(text)
    assert [r.name for r in reps] == ["first", "second"]
    assert [f.rule for f in reps[0].findings] == ["vgpr-budget"] and reps[1].findings == []


def test_flag_values():
    """The three shapes of a flag register's value and what an s_cmp can tell from them."""
    ne = lambda *c: ("ne", frozenset(c))
    assert asm_flow._not_in(frozenset({0})) == ("gt", 0) and asm_flow._not_in(frozenset({0, 1})) == ("gt", 1)
    assert asm_flow._not_in(frozenset({1})) == ne(1)
    assert asm_flow._fold("s_add_u32", ("gt", 0), 1) == ("gt", 0) == asm_flow._fold("s_add_u32", 1, ("gt", 0))      # counters do not wrap
    assert asm_flow._fold("s_add_u32", 1, ne(1)) == ne(2) and asm_flow._fold("s_sub_u32", ne(1), 1) == ne(0)
    assert asm_flow._fold("s_sub_u32", ("gt", 0), 1) is None and asm_flow._fold("s_add_u32", 0xffffffff, 1) == 0
    assert asm_flow._fold("s_and_b32", None, 0) == 0 and asm_flow._fold("s_and_b32", None, 1) is None
    assert asm_flow._fold("s_or_b32", None, ("gt", 0)) == ne(0) and asm_flow._fold("s_or_b32", 0, 5) == 5
    assert asm_flow._compare("eq", ("gt", 0), 0) is False and asm_flow._compare("eq", ("gt", 0), 1) is None
    assert asm_flow._compare("lt", 0, ("gt", 0)) is True and asm_flow._compare("ge", ("gt", 3), 2) is True
    assert asm_flow._compare("ne", ne(1), 1) is True and asm_flow._compare("eq", ne(1), 2) is None
    assert asm_flow._compare("lt", None, 3) is None


def test_a_compare_with_a_known_outcome_takes_one_arm():
    """Code behind a branch the flags exclude is never visited: its loads are not tracked, which the product test's counts turn
    into a failure instead of a silent pass."""
    rep = asm_flow.check(kernel("""
        s_mov_b32 s6, 1
        s_cmp_eq_u32 s6, 1
        s_cbranch_scc1 .Lend
        global_load_dwordx2 v[2:3], v0, s[0:1]
        v_add_u32 v4, v2, v3
        .Lend:
        s_waitcnt vmcnt(0)"""))[0]
    assert rep.findings == [] and rep.loads == 2                          # the prologue's two s_loads only
    rep = asm_flow.check(kernel("global_load_dwordx2 v[2:3], v0, s[0:1]\nv_add_u32 v4, v2, v3\ns_waitcnt vmcnt(0)"))[0]
    assert [f.rule for f in rep.findings] == ["read-pending"] and rep.loads == 3


def test_back_edge_hazard_without_flag_nodes():
    """The same loop on the plain graph (flags off): both arms of the branch get the state that arrives by the back edge."""
    for pad, want in (("", ["valu-sgpr-vmem"]), ("\n        s_nop 0", [])):
        rep = asm_flow.check(kernel(back_edge_kernel(pad)), flags=False)[0]
        assert [f.rule for f in rep.findings] == want
    swapped = back_edge_kernel("").replace("s_cbranch_scc1 .Lother", "s_cbranch_scc0 .Lother")        # the load in the taken arm's place
    assert [f.rule for f in asm_flow.check(kernel(swapped))[0].findings] == ["valu-sgpr-vmem"]


def test_mfma_distance_goes_with_the_pass_count():
    body = zero(*range(4, 24)) + "\n{mfma}\ns_nop {n}\nv_mov_b32 v30, v4"
    bf16 = "v_mfma_f32_16x16x32_bf16 v[4:7], v[8:11], v[12:15], v[4:7]"
    fp8 = "v_mfma_f32_16x16x128_f8f6f4 v[4:7], v[8:15], v[16:23], v[4:7]"
    assert findings(body.format(mfma=bf16, n=15)) == [] and [f.rule for f in findings(body.format(mfma=bf16, n=14))] == ["mfma-result"]
    assert [f.rule for f in findings(body.format(mfma=fp8, n=15))] == ["mfma-result"]
    assert findings(body.format(mfma=fp8, n=15) .replace("s_nop 15", "s_nop 15\ns_nop 2")) == []
