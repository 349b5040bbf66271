"""Dataflow checker of the generated gfx950 assembly (gen_conv1x1_asm.py, gen_conv3x3_pl_asm.py, gen_bottleneck_asm.py,
gen_bottleneck96_asm.py) -- host-side, no GPU, no assembler.

No compiler stands behind that text: every s_waitcnt count is a hand-counted constant, the assembler pads no wait-state hazard and
nothing holds the .amdhsa_* register budgets to the registers the text names.  check(text) splits one generated .s file into kernels
(global label to s_endpgm), parses every instruction into mnemonic, written and read registers and modifiers, builds the control-flow
graph (labels, s_branch, s_cbranch_scc0/1, s_endpgm) and runs three forward dataflow passes to a fixed point, so that a load issued
in one trip of a software-pipelined loop and waited for in the next is followed across the back edge.  States are kept at block
entries only; inside a block the simulation runs in place.  Where a scalar flag picks between two waits (or skips a load and, later,
its use) the graph has one node per (block, flag values): see expand_cfg.

  Pass A, memory counters.  For every register that is the destination of an outstanding VMEM load, LDS read, ds_bpermute or SMEM
    load: the number of younger operations on the same counter.  VMEM loads, VMEM stores and LDS-DMA count on vmcnt (an LDS-DMA has
    no register destination and still counts); LDS reads, LDS writes and ds_bpermute on lgkmcnt.  Both return in order:
    s_waitcnt vmcnt(n) / lgkmcnt(n) retires the destinations with at least n younger operations.  SMEM returns out of order: only
    lgkmcnt(0) retires it.  At a join a register pending on either path is pending with the smaller younger-count; counts saturate at
    the field widths (63 / 15).  Findings: `read-pending`, `write-pending` (by anything but a load on the same counter),
    `end-undrained` (s_endpgm reached with a store or LDS-DMA that no vmcnt(0) covers).
  Pass B, registers.  `read-before-write`: a VGPR, AGPR, SGPR, vcc, m0 or scc read on some path before anything wrote it (entry
    state: what the kernel descriptor enables -- user SGPRs, workgroup ids, v0, exec; a write under a partial exec is a write).
    `vgpr-budget` / `agpr-budget` / `sgpr-budget`: a register named beyond .amdhsa_accum_offset (the VGPRs end where the AGPRs
    start), .amdhsa_next_free_vgpr - .amdhsa_accum_offset, .amdhsa_next_free_sgpr.  `lds-offset`: a ds_* offset: or an immediate
    written to m0 that does not stay below .amdhsa_group_segment_fixed_size.
  Pass C, wait states the assembler does not insert (HAZARDS below: each rule with its distance and where the distance is stated).
    Distance is counted as tests/test_build_isa*.py count it: instructions in between, s_nop k counting k + 1.

Instruction classes come from the one table MNEMONICS: what the generators emit today.  A mnemonic that is not in it is the finding
`unclassified`, and so is an operand that is neither a register, `off` nor a number (-v2, |v2|: it would be skipped as a literal);
that is the only rule about unknown instructions (no list of instructions to look for or to forbid).

WHAT A GREEN RUN DOES NOT PROVE.  The checker follows registers, not addresses.  It does not prove that the LDS bytes an LDS-DMA
writes have landed (vmcnt, then the barrier) before a ds_read of the same bytes, nor that a ring buffer is free before it is
refilled, nor any ordering between workgroups.  The numeric GPU tests and the hand-counted checks of tests/test_build_isa.py and
tests/test_build_isa_c3tail.py keep covering those.  It also trusts the table: an instruction classed wrongly is checked wrongly."""
import re
from collections import namedtuple

VMCNT_MAX, LGKMCNT_MAX = 63, 15

# ---- register numbering: one integer per 32-bit register (bit position in pass B's masks) ----
V0, A0, S0 = 0, 512, 1024
VCC, M0, EXEC, SCC = S0 + 106, S0 + 124, S0 + 126, S0 + 128
_SPECIAL = {"vcc": (VCC, VCC + 1), "vcc_lo": (VCC,), "vcc_hi": (VCC + 1,), "exec": (EXEC, EXEC + 1), "exec_lo": (EXEC,),
            "exec_hi": (EXEC + 1,), "m0": (M0,), "scc": (SCC,)}
_BASE = {"v": V0, "a": A0, "s": S0}
_REG = re.compile(r"^(?:([vas])(\d+)|([vas])\[(\d+):(\d+)\]|(vcc_lo|vcc_hi|vcc|exec_lo|exec_hi|exec|m0|scc))$")


def reg_name(r):
    if r == SCC:
        return "scc"
    if r in (VCC, VCC + 1):
        return "vcc"
    if r in (EXEC, EXEC + 1):
        return "exec"
    if r == M0:
        return "m0"
    return f"s{r - S0}" if r >= S0 else f"a{r - A0}" if r >= A0 else f"v{r}"


# ---- the one table: mnemonic -> (class, destination operands, implicit reads, implicit writes) ----
VALU, TRANS, MFMA, SALU, VLOAD, VSTORE, LDSDMA, LREAD, LWRITE, SMEM, WAIT, NOP, BARRIER, BRANCH = (
    "VALU", "transcendental", "MFMA", "SALU", "VMEM load", "VMEM store", "LDS-DMA", "LDS read", "LDS write", "SMEM", "wait", "nop",
    "barrier", "branch")
MNEMONICS = {}


def _add(cls, names, ndst=1, iread=(), iwrite=()):
    for n in names.split():
        MNEMONICS[n] = (cls, ndst, tuple(iread), tuple(iwrite))


_add(VALU, "v_accvgpr_read_b32 v_add3_u32 v_add_f32_e64 v_add_u32 v_and_b32 v_ashrrev_i32 v_bfe_u32 v_bfrev_b32 v_cndmask_b32 "
           "v_cvt_f32_i32 v_cvt_i32_f32 v_cvt_pk_bf16_f32 v_cvt_pk_f32_fp8_e32 v_cvt_pk_f32_fp8_sdwa v_lshl_add_u32 v_lshl_or_b32 "
           "v_lshlrev_b32 v_lshrrev_b32 v_mad_u32_u24 v_min_i32 v_mov_b32 v_mul_f32 v_mul_f32_e64 v_mul_lo_u32 v_mul_u32_u24 "
           "v_pk_add_f32 v_pk_mul_f32 v_sub_u32 v_subrev_u32 v_xad_u32 v_xor_b32 v_readfirstlane_b32 "
           "v_cmp_eq_u32 v_cmp_gt_i32 v_cmp_gt_u32 v_cmp_le_i32 v_cmp_lt_u32")
_add(VALU, "v_add_co_u32 v_addc_co_u32 v_subbrev_co_u32 v_mad_u64_u32", ndst=2)          # vdst, carry out
_add(VALU, "v_permlane16_swap_b32 v_permlane32_swap_b32", ndst=2)                          # both operands are read and written
_add(TRANS, "v_exp_f32 v_rcp_f32")
_add(MFMA, "v_mfma_f32_16x16x32_bf16 v_mfma_f32_16x16x128_f8f6f4")
_add(SALU, "s_mov_b32 s_mov_b64 s_mul_i32 s_mul_hi_u32")
_add(SALU, "s_add_u32 s_sub_u32 s_sub_i32 s_and_b32 s_and_b64 s_andn2_b64 s_or_b32 s_or_b64 s_xor_b32 s_lshl_b32 s_lshr_b32 s_min_u32",
     iwrite=(SCC,))
_add(SALU, "s_addc_u32 s_subb_u32", iread=(SCC,), iwrite=(SCC,))
_add(SALU, "s_cselect_b32 s_cselect_b64", iread=(SCC,))
_add(SALU, "s_cmp_eq_u32 s_cmp_ge_u32 s_cmp_gt_u32 s_cmp_le_u32 s_cmp_lg_u32 s_cmp_lt_u32 s_bitcmp0_b32", ndst=0, iwrite=(SCC,))
_add(SALU, "s_and_saveexec_b64", iread=(EXEC, EXEC + 1), iwrite=(EXEC, EXEC + 1, SCC))
_add(VLOAD, "buffer_load_dwordx2 buffer_load_dwordx4 global_load_dwordx2 global_load_dwordx4")   # with the `lds` modifier: LDS-DMA
_add(LDSDMA, "global_load_lds_dwordx4", ndst=0, iread=(M0,))
_add(VSTORE, "buffer_store_dwordx2 buffer_store_dwordx4 global_store_dwordx2 global_store_dwordx4", ndst=0)
_add(LREAD, "ds_read_b128 ds_bpermute_b32")
_add(LWRITE, "ds_write_b64 ds_write_b128", ndst=0)
_add(SMEM, "s_load_dword s_load_dwordx2 s_load_dwordx4 s_load_dwordx8 s_memtime s_memrealtime")
_add(WAIT, "s_waitcnt", ndst=0)
_add(NOP, "s_nop", ndst=0)
_add(BARRIER, "s_barrier", ndst=0)
_add(BRANCH, "s_branch s_endpgm", ndst=0)
_add(BRANCH, "s_cbranch_scc0 s_cbranch_scc1", ndst=0, iread=(SCC,))
_VECTOR = (VALU, TRANS, MFMA)
_VMEM = (VLOAD, VSTORE, LDSDMA)

# ---- pass C: rule -> (wait states required between producer and consumer, where the distance is stated) ----
HAZARDS = {
    # MFMA D -> a reader (or VALU writer) that is not an MFMA of the same kind: v_accvgpr_read, VALU, store data, address.  The distance
    # goes with the MFMA's pass count, MFMA_STATES below.  Stated: gen_conv3x3_pl_asm.py header "MFMA result -> VALU read up to 19 (s_nop 15
    # twice before the epilogue)": the 16-pass case, here v_mfma_f32_16x16x128_f8f6f4 on fp8.  For the 8-pass v_mfma_f32_16x16x32_bf16 the
    # gen_conv1x1 / gen_bottleneck / gen_bottleneck96 headers say "s_nop 15" = 16 and cdna_hip_programming.md 5.7 item 2 says 12 ("8-pass
    # XDL: 12 states"): the larger, 16, applies -- it is what the generators that emit this MFMA promise in their own headers.
    "mfma-result": (19, "gen_conv3x3_pl_asm.py header: up to 19 (16-pass); 8-pass: 16 (s_nop 15, the other headers) over 12 (guide 5.7 item 2)"),
    # v_exp / v_rcp result -> a consumer that is not itself transcendental.  Stated: planar header "transcendental -> consumer 1";
    # the other headers "independent instructions in between" (at least one).
    "trans-result": (1, "gen_conv3x3_pl_asm.py header: 1; other headers: independent instructions in between"),
    # SALU write of m0 -> LDS-DMA.  Stated: all four headers "s_mov m0 -> LDS-DMA (s_nop 0)" = 1; guide 5.7 recipe: s_nop 0.
    "m0-dma": (1, "all four generator headers: s_nop 0; guide 5.7 LDS-DMA recipe"),
    # VALU write of a VGPR -> v_readfirstlane reading it.  Stated: conv1x1 / c48 / c96 headers "s_nop 1" = 2; planar header and guide
    # 5.7 item 2 say 1 (s_nop 0).  The larger applies: three of the four generators pad two and say so.
    "valu-readfirstlane": (2, "gen_conv1x1/bottleneck/bottleneck96 headers: s_nop 1; smaller: 1 (planar header, guide 5.7 item 2)"),
    # VALU write of a VGPR -> v_permlane16/32_swap reading it.  Stated: guide T21 "2 wait states"; gen_bottleneck_asm.py emit_tail_gemm.
    "valu-permlane": (2, "guide 5.5 T21 permlane-swap paragraph: 2 wait states; gen_bottleneck_asm.py emit_tail_gemm"),
    # VALU-written SGPR (v_readfirstlane, v_cmp, carry out) -> VMEM instruction reading it.  Stated: planar header 5; c48 header
    # "s_nop 4" = 5; guide 5.7 item 2 "s_nop 4".
    "valu-sgpr-vmem": (5, "gen_conv3x3_pl_asm.py header: 5; gen_bottleneck_asm.py header: s_nop 4; guide 5.7 item 2"),
    # store of more than 8 bytes -> VALU write of its data registers.  Stated: gen_bottleneck_asm.py W16 note "TWO wait states";
    # guide 5.7 item 1 "ends with s_nop 1"; tests/test_build_isa_c3tail.py checks the two instructions behind the store.
    "store16-data": (2, "gen_bottleneck_asm.py W16 note: two wait states; guide 5.7 item 1: s_nop 1"),
}

Finding = namedtuple("Finding", "kernel line rule text detail")     # line: 1-based, counted from the kernel's label


class Ins:
    __slots__ = ("line", "text", "mn", "cls", "reads", "writes", "rmask", "wmask", "mods", "imm", "target", "data", "ops", "bad")

    def __repr__(self):
        return f"<{self.line}: {self.text}>"


_opcache = {}
_LITERAL = re.compile(r"^-?(0x[0-9a-fA-F]+|\d+(\.\d+)?)$")


def _operand(tok):
    """Registers of one operand (a tuple; empty for literals, `off`, labels)."""
    r = _opcache.get(tok)
    if r is None:
        m = _REG.match(tok)
        if not m:
            r = ()
        elif m.group(1):
            r = (_BASE[m.group(1)] + int(m.group(2)),)
        elif m.group(3):
            lo, hi = int(m.group(4)), int(m.group(5))
            r = tuple(range(_BASE[m.group(3)] + lo, _BASE[m.group(3)] + hi + 1))
        else:
            r = _SPECIAL[m.group(6)]
        _opcache[tok] = r
    return r


def _mask(regs):
    m = 0
    for r in regs:
        m |= 1 << r
    return m


def parse_instruction(text, line=0):
    """One instruction line (comment already removed, stripped) -> Ins.  An unknown mnemonic gets cls None."""
    ins = Ins()
    ins.line, ins.text = line, text
    mn, _, rest = text.partition(" ")
    ins.mn = mn
    ins.mods, ins.imm, ins.target, ins.data, ins.ops, ins.bad = (), None, None, (), (), None
    ent = MNEMONICS.get(mn)
    if ent is None:
        ins.cls, ins.reads, ins.writes, ins.rmask, ins.wmask = None, (), (), 0, 0
        return ins
    cls, ndst, iread, iwrite = ent
    rest = rest.strip()
    if cls == WAIT:
        ins.imm = {k: int(n) for k, n in re.findall(r"(vmcnt|lgkmcnt)\((\d+)\)", rest)}
        ops = []
    elif cls == NOP:
        ins.imm = int(rest, 0)
        ops = []
    elif cls == BRANCH:
        ins.target = rest or None
        ops = []
    else:
        ops = [o.strip() for o in rest.split(",")] if rest else []
        if ops:
            last = ops[-1].split()
            ops[-1] = last[0]
            ins.mods = tuple(last[1:])
    if cls == VLOAD and "lds" in ins.mods:
        cls, ndst, iread = LDSDMA, 0, (M0,)
    ins.cls, ins.ops = cls, tuple(ops)
    regs = [_operand(o) for o in ops]
    for o in ops:                                 # -v2, |v2|, neg(..), a symbol: not read as a register, so it must not pass as a literal
        if not _REG.match(o) and o != "off" and not _LITERAL.match(o):
            ins.bad = o
    writes = [r for o in regs[:ndst] for r in o]
    reads = [r for o in regs[ndst:] for r in o]
    if mn.startswith("v_permlane"):
        reads += writes
    if mn == "v_cndmask_b32" and len(ops) == 3:
        reads += [VCC, VCC + 1]
    if cls == VSTORE:
        ins.data = regs[0] if mn.startswith("buffer_") else regs[1]
    if cls == SALU and ndst and ops and ops[0] == "m0" and len(ops) > 1:
        for o in ops[1:]:
            if re.match(r"^(0x[0-9a-fA-F]+|\d+)$", o):
                ins.imm = int(o, 0)
    ins.reads, ins.writes = tuple(reads) + iread, tuple(writes) + iwrite
    ins.rmask, ins.wmask = _mask(ins.reads), _mask(ins.writes)
    return ins


Kernel = namedtuple("Kernel", "name ins labels desc text")


def split_kernels(text):
    """The kernels of one .s file: global label .. s_endpgm, each with the .amdhsa_* values of its descriptor."""
    descs, cur = {}, None
    for l in text.split("\n"):
        t = l.strip()
        if t.startswith(".amdhsa_kernel "):
            cur = descs.setdefault(t.split()[1], {})
        elif t.startswith(".end_amdhsa_kernel"):
            cur = None
        elif cur is not None and t.startswith(".amdhsa_"):
            k, _, val = t.partition(" ")
            cur[k[len(".amdhsa_"):]] = int(val.split(";")[0], 0)
    kernels, name, ins, labels, raw = [], None, None, None, None
    for l in text.split("\n"):
        t = l.split(";", 1)[0].strip()
        if not t:
            continue
        if name is None:
            if t.endswith(":") and not t.startswith(".") and " " not in t:
                name, ins, labels, raw = t[:-1], [], {}, [l]
            continue
        raw.append(l)
        if t.endswith(":") and " " not in t:
            labels[t[:-1]] = len(ins)
            continue
        if t.startswith("."):
            continue
        ins.append(parse_instruction(t, len(raw)))
        if t == "s_endpgm":
            kernels.append(Kernel(name, ins, labels, descs.get(name, {}), "\n".join(raw)))
            name = None
    return kernels


def build_cfg(k, cuts=()):
    """Basic blocks [(start, end)] of a kernel and their successors (block numbers), and the branches to unknown labels.
    `cuts`: instructions after which a block must end as well."""
    n = len(k.ins)
    leaders = {0} | {i + 1 for i in cuts if i + 1 < n}
    for i, x in enumerate(k.ins):
        if x.cls == BRANCH:
            if i + 1 < n:
                leaders.add(i + 1)
            if x.target is not None and x.target in k.labels and k.labels[x.target] < n:
                leaders.add(k.labels[x.target])
    for pos in k.labels.values():
        if pos < n:
            leaders.add(pos)
    starts = sorted(leaders)
    blocks = [(s, e) for s, e in zip(starts, starts[1:] + [n])]
    at = {s: b for b, (s, _) in enumerate(blocks)}
    succs, bad = [], []
    for b, (s, e) in enumerate(blocks):
        x = k.ins[e - 1]
        out = []
        if x.cls == BRANCH and x.mn != "s_endpgm":
            if x.target in k.labels and k.labels[x.target] < n:
                out.append(at[k.labels[x.target]])
            else:
                bad.append(x)
        if (x.cls != BRANCH or x.mn.startswith("s_cbranch")) and e < n:
            out.append(at[e])
        succs.append(out)
    return blocks, succs, bad


# ---- scalar flags: the paths a scalar condition excludes ----
# The generators pick between two s_waitcnt immediates (or skip a load and, later, its use) by a scalar flag: `after_epi`, "last chunk",
# "a tile follows".  Merging all paths into one state per block would hold the wait of one arm against the loads of the other.  So the
# passes run on a graph whose nodes are (block, values of the flag registers): constants are folded through s_mov / s_add / s_sub /
# s_and / s_or / s_xor / s_cselect, an s_cmp with a known outcome takes one arm, one with an unknown outcome that feeds a branch or a
# flag forks into both outcomes (refining the compared register: == c, or != c), and only the registers such a compare can depend on,
# where they are still live, tell nodes apart.  Values: an integer, ("gt", m) = above m (a counter that has left the values it is
# compared with; counters are taken not to wrap), ("ne", {c ..}) = none of these.  What this cannot see -- a relation between two
# unknown registers, such as chunk + 1 == nchunks here and chunk < nchunks there -- stays one merged path.
_M32 = 0xffffffff
_CMP = {"s_cmp_eq_u32": "eq", "s_cmp_lg_u32": "ne", "s_cmp_lt_u32": "lt", "s_cmp_le_u32": "le", "s_cmp_gt_u32": "gt", "s_cmp_ge_u32": "ge"}
_FOLD = ("s_mov_b32", "s_add_u32", "s_sub_u32", "s_and_b32", "s_or_b32", "s_xor_b32", "s_cselect_b32")
_INT = re.compile(r"^-?(0x[0-9a-fA-F]+|\d+)$")
MAX_NODES = 40000


def _imm(tok):
    return int(tok, 0) & _M32 if _INT.match(tok) else None


def _val(env, tok):
    v = _imm(tok)
    if v is None:
        r = _operand(tok)
        if len(r) == 1:
            return env.get(r[0])
    return v


def _not_in(consts):
    """The value "none of these": ("gt", m) when they are exactly 0 .. m (registers are unsigned), else ("ne", consts)."""
    return ("gt", len(consts) - 1) if consts == frozenset(range(len(consts))) else ("ne", frozenset(consts))


def _nonzero(v):
    return v is not None and (v != 0 if isinstance(v, int) else v[0] == "gt" or 0 in v[1])


def _fold(mn, a, b):
    ia, ib = isinstance(a, int), isinstance(b, int)
    if mn == "s_add_u32" and ia and not ib:
        a, b, ia, ib = b, a, ib, ia
    if mn in ("s_add_u32", "s_sub_u32"):
        sign = 1 if mn == "s_add_u32" else -1
        if ia and ib:
            return (a + sign * b) & _M32
        if ib and a is not None and a[0] == "ne":
            return ("ne", frozenset((c + sign * b) & _M32 for c in a[1]))
        if ib and a is not None and a[0] == "gt" and sign == 1 and b < 1 << 31:
            return a
        return None
    if mn == "s_and_b32":
        return a & b if ia and ib else 0 if a == 0 or b == 0 else None
    if mn == "s_or_b32":
        return a | b if ia and ib else b if a == 0 else a if b == 0 else ("ne", frozenset((0,))) if _nonzero(a) or _nonzero(b) else None
    return a ^ b if ia and ib else None


def _compare(kind, a, b):
    """Outcome of an s_cmp (True / False), None when the values do not decide it."""
    if a is None or b is None:
        return None
    if isinstance(a, int) and isinstance(b, int):
        return {"eq": a == b, "ne": a != b, "lt": a < b, "le": a <= b, "gt": a > b, "ge": a >= b}[kind]
    if isinstance(a, int):
        return _compare({"eq": "eq", "ne": "ne", "lt": "gt", "le": "ge", "gt": "lt", "ge": "le"}[kind], b, a)
    if not isinstance(b, int):
        return None
    if a[0] == "gt":
        return {"eq": False, "ne": True, "lt": False, "le": False, "gt": True, "ge": True}[kind] if b <= a[1] else None
    return {"eq": False, "ne": True}.get(kind) if b in a[1] else None


def _scalar_slice(k):
    """(registers an s_cmp that decides a branch can depend on, those s_cmp instructions)."""
    ins = k.ins

    def producer(i):
        for j in range(i - 1, -1, -1):
            if SCC in ins[j].writes:
                return j if ins[j].mn in _CMP else None
        return None

    rel, forks, new = set(), set(), set()

    def want(j):
        if j is not None and j not in forks:
            forks.add(j)
            new.update(r for r in ins[j].reads if r >= S0)

    for i, x in enumerate(ins):
        if x.mn.startswith("s_cbranch"):
            want(producer(i))
    while not new <= rel:
        rel |= new
        for i, x in enumerate(ins):
            if x.mn in _FOLD and x.writes[0] in rel:
                new.update(r for r in x.reads if r >= S0 and r != SCC)
                if x.mn == "s_cselect_b32":
                    want(producer(i))
    return rel, forks


def expand_cfg(k):
    """The control-flow graph with one node per (block, flag values): ([(start, end)], successors, branches to unknown labels)."""
    ins = k.ins
    rel, forks = _scalar_slice(k)
    blocks, succs, bad = build_cfg(k, forks)
    if not forks:
        return blocks, succs, bad
    relmask = _mask(rel | {SCC})
    widen = {}
    for x in ins:
        if x.mn in _CMP:
            for a, b in (x.ops, x.ops[::-1]):
                r, c = _operand(a), _imm(b)
                if len(r) == 1 and c is not None:
                    widen[r[0]] = max(widen.get(r[0], 0), c)
    # liveness of the flag registers: a node is told apart only by values something below it can still read
    use, kill = [], []
    for s, e in blocks:
        u = d = 0
        for i in range(s, e):
            u |= ins[i].rmask & relmask & ~d
            d |= ins[i].wmask & relmask
        use.append(u)
        kill.append(d)
    live = list(use)
    changed = True
    while changed:
        changed = False
        for b in range(len(blocks) - 1, -1, -1):
            out = 0
            for t in succs[b]:
                out |= live[t]
            new = use[b] | (out & ~kill[b])
            if new != live[b]:
                live[b], changed = new, True
    at = {s: b for b, (s, _) in enumerate(blocks)}
    nodes, order, edges, work = {}, [], [], []

    def node(b, env):
        env = {r: v for r, v in env.items() if live[b] >> r & 1}
        key = (b, frozenset(env.items()))
        n = nodes.get(key)
        if n is None:
            n = nodes[key] = len(order)
            order.append((b, env))
            edges.append(())
            work.append(n)
            if n > MAX_NODES:
                raise RuntimeError(f"{k.name}: more than {MAX_NODES} (block, flag values) nodes")
        return n

    node(0, {})
    while work:
        n = work.pop()
        b, env = order[n]
        env = dict(env)
        s, e = blocks[b]
        out = None
        for i in range(s, e):
            x = ins[i]
            mn = x.mn
            if mn in _CMP:
                a, c = _val(env, x.ops[0]), _val(env, x.ops[1])
                r = _compare(_CMP[mn], a, c)
                if r is not None:
                    env[SCC] = int(r)
                elif i in forks and i == e - 1:
                    out = []
                    for outcome in (1, 0):
                        env2 = dict(env)
                        env2[SCC] = outcome
                        kind = _CMP[mn]
                        if kind in ("eq", "ne"):
                            for p, q in (x.ops, x.ops[::-1]):
                                reg, cst = _operand(p), _imm(q)
                                if len(reg) == 1 and reg[0] in rel and cst is not None:
                                    cur = env.get(reg[0])
                                    if (kind == "eq") == bool(outcome):
                                        env2[reg[0]] = cst
                                    elif cur is None or cur[0] == "ne":
                                        env2[reg[0]] = _not_in((cur[1] if cur else frozenset()) | {cst})
                        out += [node(t, env2) for t in succs[b]]
                else:
                    env.pop(SCC, None)
            elif mn in _FOLD and x.writes[0] in rel:
                d = x.writes[0]
                if mn == "s_mov_b32":
                    v = _val(env, x.ops[1])
                elif mn == "s_cselect_b32":
                    a, c, scc = _val(env, x.ops[1]), _val(env, x.ops[2]), env.get(SCC)
                    v = (a if scc else c) if scc is not None else a if a == c else None
                else:
                    v = _fold(mn, _val(env, x.ops[1]), _val(env, x.ops[2]))
                    env.pop(SCC, None)
                    if isinstance(v, int) and mn == "s_add_u32" and x.ops[0] in x.ops[1:] and v > widen.get(d, 0):
                        v = ("gt", widen.get(d, 0))
                if v is None:
                    env.pop(d, None)
                else:
                    env[d] = v
            elif x.writes:
                for r in x.writes:
                    if r >= S0:
                        env.pop(r, None)
        if out is None:
            x = ins[e - 1]
            scc = env.get(SCC)
            if x.mn.startswith("s_cbranch") and scc is not None and x.target in k.labels and k.labels[x.target] < len(ins):
                taken = scc == (1 if x.mn.endswith("scc1") else 0)
                out = [node(at[k.labels[x.target]] if taken else at[e], env)] if taken or e < len(ins) else []
            else:
                out = [node(t, env) for t in succs[b]]
        edges[n] = out
    expand_cfg.last = order                 # (block, flag values) per node, for whoever debugs a finding
    return [blocks[b] for b, _ in order], edges, bad


def _fixed_point(blocks, succs, entry, transfer, merge):
    """Forward worklist: states at block entries only; transfer(block number, state) -> state at the block's end (a new object)."""
    state = [None] * len(blocks)
    state[0] = entry
    work = [0]
    while work:
        b = work.pop()
        out = transfer(b, state[b])
        for t in succs[b]:
            if state[t] is None:
                state[t] = out if len(succs[b]) == 1 else _copy(out)
                changed = True
            else:
                changed = merge(state[t], out)
            if changed and t not in work:
                work.append(t)
    return state


def _copy(st):
    if isinstance(st, tuple):
        return tuple(_copy(x) for x in st)
    if isinstance(st, list):
        return [_copy(x) for x in st]
    if isinstance(st, dict):                    # pass C's state is a dict of dicts: two successors must not share the inner ones
        return {key: _copy(x) for key, x in st.items()}
    if isinstance(st, set):
        return set(st)
    return st


class KernelReport:
    def __init__(self, name):
        self.name, self.findings, self.loads, self.waits, self.sites, self.instructions, self.nodes = name, [], 0, 0, {}, 0, 0

    def rules(self):
        return sorted({f.rule for f in self.findings})


def _min_merge(into, new):
    ch = False
    for r, y in new.items():
        o = into.get(r)
        if o is None or y < o:
            into[r] = y
            ch = True
    return ch


# ---- pass A ----
def _pass_a(k, blocks, succs, rep, found):
    ins = k.ins
    loads, waits = set(), set()

    def transfer(b, st):
        vm0, lg0, sm0, st0 = st
        vmc = lgc = 0
        vm = {r: -y for r, y in vm0.items()}          # register -> counter value right after its load: younger = counter - that
        lg = {r: -y for r, y in lg0.items()}
        sm = set(sm0)
        store = None if st0 is None else -st0         # the youngest store / LDS-DMA, same encoding
        for i in range(*blocks[b]):
            x = ins[i]
            cls = x.cls
            if vm or lg or sm:
                for r in x.reads:
                    if r in vm or r in lg or r in sm:
                        found(x, "read-pending", f"{reg_name(r)} is read while the load that fills it may still be in flight")
                        vm.pop(r, None), lg.pop(r, None), sm.discard(r)
                for r in x.writes:
                    if (r in vm and cls != VLOAD) or (r in lg and cls != LREAD) or r in sm:
                        found(x, "write-pending", f"{reg_name(r)} is written while a load into it may still be in flight")
                        vm.pop(r, None), lg.pop(r, None), sm.discard(r)
            if cls == VLOAD:
                vmc += 1
                loads.add(i)
                for r in x.writes:
                    vm[r] = vmc
            elif cls == VSTORE or cls == LDSDMA:
                vmc += 1
                store = vmc
            elif cls == LREAD:
                lgc += 1
                loads.add(i)
                for r in x.writes:
                    lg[r] = lgc
            elif cls == LWRITE:
                lgc += 1
            elif cls == SMEM:
                loads.add(i)
                sm.update(x.writes)
            elif cls == WAIT:
                waits.add(i)
                n = x.imm.get("vmcnt")
                if n is not None:
                    if vm:
                        vm = {r: c for r, c in vm.items() if vmc - c < n}
                    if store is not None and vmc - store >= n:
                        store = None
                n = x.imm.get("lgkmcnt")
                if n is not None:
                    if lg:
                        lg = {r: c for r, c in lg.items() if lgc - c < n}
                    if n == 0:
                        sm.clear()
            elif x.mn == "s_endpgm" and store is not None:
                found(x, "end-undrained", "s_endpgm is reached with a store or LDS-DMA that no s_waitcnt vmcnt(0) covers")
        return ({r: min(vmc - c, VMCNT_MAX) for r, c in vm.items()}, {r: min(lgc - c, LGKMCNT_MAX) for r, c in lg.items()}, sm,
                None if store is None else min(vmc - store, VMCNT_MAX))

    def merge(into, new):
        ch = _min_merge(into[0], new[0]) | _min_merge(into[1], new[1])
        if not new[2] <= into[2]:
            into[2].update(new[2])
            ch = True
        if new[3][0] is not None and (into[3][0] is None or new[3][0] < into[3][0]):
            into[3][0] = new[3][0]
            ch = True
        return ch

    # the store count sits in a one-element list so that merge can update it in place
    def transfer_boxed(b, st):
        out = transfer(b, (st[0], st[1], st[2], st[3][0]))
        return (out[0], out[1], out[2], [out[3]])

    states = _fixed_point(blocks, succs, ({}, {}, set(), [None]), transfer_boxed, merge)
    rep.loads, rep.waits = len(loads), len(waits)
    return states


# ---- pass B ----
def _entry_registers(desc):
    n = desc.get("user_sgpr_count")
    if n is None:
        n = 2 * desc.get("user_sgpr_kernarg_segment_ptr", 0)
    regs = [S0 + i for i in range(n)]
    for ax, default in (("x", 1), ("y", 0), ("z", 0)):
        if desc.get("system_sgpr_workgroup_id_" + ax, default):
            regs.append(S0 + n)
            n += 1
    return regs + [V0, EXEC, EXEC + 1]              # gfx950 packs the work-item ids into v0


def _pass_b(k, blocks, succs, rep, found):
    ins = k.ins
    top = -1

    def transfer(b, defined):
        for i in range(*blocks[b]):
            x = ins[i]
            miss = x.rmask & ~defined
            if miss:
                r = (miss & -miss).bit_length() - 1
                found(x, "read-before-write", f"{reg_name(r)} is read on a path on which nothing wrote it")
                defined |= miss
            defined |= x.wmask
        return defined

    state = [top] * len(blocks)
    state[0] = _mask(_entry_registers(k.desc))
    work, seen = [0], {0}
    while work:
        b = work.pop()
        out = transfer(b, state[b])
        for t in succs[b]:
            new = state[t] & out
            if new != state[t] or t not in seen:
                state[t] = new
                seen.add(t)
                if t not in work:
                    work.append(t)
    # budgets and static LDS offsets
    d = k.desc
    lim = {"vgpr-budget": (V0, d.get("accum_offset", d.get("next_free_vgpr", 0)), ".amdhsa_accum_offset"),
           "agpr-budget": (A0, d.get("next_free_vgpr", 0) - d.get("accum_offset", d.get("next_free_vgpr", 0)),
                           ".amdhsa_next_free_vgpr - .amdhsa_accum_offset"),
           "sgpr-budget": (S0, d.get("next_free_sgpr", 0), ".amdhsa_next_free_sgpr")}
    lds = d.get("group_segment_fixed_size", 0)
    for x in ins:
        for r in x.reads + x.writes:
            rule = "sgpr-budget" if S0 <= r < VCC else "agpr-budget" if A0 <= r < S0 else "vgpr-budget" if r < A0 else None
            if rule and r - lim[rule][0] >= lim[rule][1]:
                found(x, rule, f"{reg_name(r)} is beyond {lim[rule][2]} = {lim[rule][1]}")
        if x.cls in (LREAD, LWRITE):
            for m in x.mods:
                if m.startswith("offset:") and int(m[7:], 0) >= lds:
                    found(x, "lds-offset", f"{m} is not below .amdhsa_group_segment_fixed_size = {lds}")
        elif x.cls == SALU and x.imm is not None and M0 in x.writes and x.imm >= lds:
            found(x, "lds-offset", f"m0 immediate {x.imm} is not below .amdhsa_group_segment_fixed_size = {lds}")


# ---- pass C ----
_KINDS = ("trans", "valu", "vsgpr", "m0", "st16")
_WINDOW = {"trans": HAZARDS["trans-result"][0], "valu": max(HAZARDS["valu-readfirstlane"][0], HAZARDS["valu-permlane"][0]),
           "vsgpr": HAZARDS["valu-sgpr-vmem"][0], "m0": HAZARDS["m0-dma"][0], "st16": HAZARDS["store16-data"][0]}
_MFMA_N = HAZARDS["mfma-result"][0]
MFMA_STATES = {"v_mfma_f32_16x16x32_bf16": 16, "v_mfma_f32_16x16x128_f8f6f4": _MFMA_N}      # 8-pass, 16-pass; any other MFMA: the largest


def _pass_c(k, blocks, succs, rep, found):
    ins = k.ins
    sites = {r: set() for r in HAZARDS}
    n_rfl, n_perm, n_vs = HAZARDS["valu-readfirstlane"][0], HAZARDS["valu-permlane"][0], HAZARDS["valu-sgpr-vmem"][0]

    def window(kind):
        return MFMA_STATES.get(kind, _MFMA_N) if kind.startswith("v_mfma") else _WINDOW[kind]

    def transfer(b, st):
        # st: kind -> {register: wait states since the write}; inside the block: register -> position right after the producer
        pos = 0
        d = {kind: {r: -age for r, age in regs.items()} for kind, regs in st.items()}
        for kind in _KINDS:
            d.setdefault(kind, {})
        trans, valu, vsgpr, m0, st16 = (d[kind] for kind in _KINDS)
        mf = {kind: regs for kind, regs in d.items() if kind.startswith("v_mfma")}
        for i in range(*blocks[b]):
            x = ins[i]
            cls, mn = x.cls, x.mn
            if cls is None:
                pos += 1
                continue
            vector = cls in _VECTOR
            for kind, regs in mf.items():
                if regs and not (cls == MFMA and mn == kind):
                    need = MFMA_STATES.get(kind, _MFMA_N)
                    for r in x.reads + (x.writes if vector else ()):
                        c = regs.get(r)
                        if c is not None and pos - c < need:
                            found(x, "mfma-result", f"{reg_name(r)}: {pos - c} wait states after the {kind} that writes it, {need} needed")
                            break
            if trans and cls != TRANS:
                for r in x.reads:
                    c = trans.get(r)
                    if c is not None and pos - c < _WINDOW["trans"]:
                        found(x, "trans-result", f"{reg_name(r)}: read right behind the transcendental that writes it")
                        break
            if cls == LDSDMA:
                sites["m0-dma"].add(i)
                c = m0.get(M0)
                if c is not None and pos - c < _WINDOW["m0"]:
                    found(x, "m0-dma", "LDS-DMA right behind the write of m0")
            if mn == "v_readfirstlane_b32" or mn.startswith("v_permlane"):
                rule, need = ("valu-readfirstlane", n_rfl) if mn[2] == "r" else ("valu-permlane", n_perm)
                sites[rule].add(i)
                for r in x.reads:
                    c = valu.get(r)
                    if c is not None and pos - c < need:
                        found(x, rule, f"{reg_name(r)}: {pos - c} wait states after the VALU write, {need} needed")
                        break
            if cls in _VMEM:
                sites["valu-sgpr-vmem"].add(i)
                if vsgpr:
                    for r in x.reads:
                        c = vsgpr.get(r)
                        if c is not None and pos - c < n_vs:
                            found(x, "valu-sgpr-vmem", f"{reg_name(r)}: {pos - c} wait states after the VALU that writes it, {n_vs} needed")
                            break
            if st16 and vector:
                for r in x.writes:
                    c = st16.get(r)
                    if c is not None and pos - c < _WINDOW["st16"]:
                        found(x, "store16-data", f"{reg_name(r)}: data of a 16-byte store written {pos - c} wait states behind it")
                        break
            # this instruction as a producer
            pos += x.imm + 1 if cls == NOP else 1
            if x.writes:
                for regs in d.values():
                    if regs:
                        for r in x.writes:
                            regs.pop(r, None)
                if cls == MFMA:
                    sites["mfma-result"].add(i)
                    regs = mf.get(mn)
                    if regs is None:
                        regs = mf[mn] = d[mn] = {}
                    for r in x.writes:
                        regs[r] = pos
                elif vector:
                    if cls == TRANS:
                        sites["trans-result"].add(i)
                    for r in x.writes:
                        if r >= S0:
                            vsgpr[r] = pos
                        else:
                            valu[r] = pos
                            if cls == TRANS:
                                trans[r] = pos
                    if len(valu) > 64:
                        for kind in ("valu", "trans", "vsgpr"):
                            w = _WINDOW[kind]
                            for r in [r for r, c in d[kind].items() if pos - c >= w]:
                                del d[kind][r]
                elif cls == SALU and M0 in x.writes:
                    m0[M0] = pos
            if cls == VSTORE and len(x.data) > 2:
                sites["store16-data"].add(i)
                for r in x.data:
                    st16[r] = pos
        return {kind: {r: pos - c for r, c in regs.items() if pos - c < window(kind)} for kind, regs in d.items()}

    def merge(into, new):
        ch = False
        for kind, regs in new.items():
            if regs:
                ch |= _min_merge(into.setdefault(kind, {}), regs)
        return ch

    _fixed_point(blocks, succs, {}, transfer, merge)
    rep.sites = {r: len(s) for r, s in sites.items()}


def check_kernel(k, passes="ABC", flags=True):
    rep = KernelReport(k.name)
    rep.instructions = len(k.ins)
    seen = set()

    def found(x, rule, detail):
        if (x.line, rule) not in seen:
            seen.add((x.line, rule))
            rep.findings.append(Finding(k.name, x.line, rule, x.text, detail))

    for x in k.ins:
        if x.cls is None:
            found(x, "unclassified", f"unclassified instruction: {x.mn} is not in the table")
        elif x.bad is not None:
            found(x, "unclassified", f"unclassified operand: {x.bad} is neither a register, `off` nor a number")
    blocks, succs, bad = expand_cfg(k) if flags else build_cfg(k)
    rep.nodes = len(blocks)
    for x in bad:
        found(x, "unclassified", f"branch to the unknown label {x.target}")
    if "A" in passes:
        _pass_a(k, blocks, succs, rep, found)
    if "B" in passes:
        _pass_b(k, blocks, succs, rep, found)
    if "C" in passes:
        _pass_c(k, blocks, succs, rep, found)
    rep.findings.sort(key=lambda f: (f.line, f.rule))
    return rep


def check(text, passes="ABC", flags=True):
    """All kernels of one .s file -> [KernelReport]."""
    return [check_kernel(k, passes, flags) for k in split_kernels(text)]
