"""The generated assembly kernels under tests/asm_flow.py: waits, register use and wait-state hazards by dataflow -- no GPU needed.

Every kernel of the four default generations (no AQ_GEN_* variable set) must come out of the checker without a finding outside the
waivers below; the checker must have tracked every load and evaluated every wait of the kernel's text (a vacuous pass fails); the
kernel lists are spelled out, so a kernel that drops out of the check is a change of this file.  Mutations of the real text (one
regular-expression edit to one kernel) must each produce the expected finding in that kernel and leave the others' text alone.

What a green run does not prove is in the docstring of tests/asm_flow.py: above all that LDS bytes written by an LDS-DMA have landed
before they are read.  tests/test_build_isa.py, tests/test_build_isa_c3tail.py and the numeric GPU tests keep covering that.

Recorded by `python tests/test_build_isa_flow.py` (recorded, not asserted):

  generator  kernels  instructions   loads   waits  hazard sites  waived findings   raised vmcnt flagged   raised lgkmcnt flagged
  conv1x1          4          5418     252     190          1612                0       28 of    38            134 of   152
  planar          46        226027   14222    6466         50448             4938      910 of  1441           3897 of  5025
  c48              3          8226     710     211          3124               20       21 of    33            171 of   178
  c96              2          4546     505     256          1584                6        6 of    13            236 of   243
  the same over the 18 kernels that are neither stamped nor ablation builds (2 / 13 / 2 / 1):
  conv1x1          2                                                                    14 of    18             66 of    70
  planar          13                                                                   340 of   359           1394 of  1433
  c48              2                                                                    15 of    23            118 of   122
  c96              1                                                                     3 of     6            116 of   119

  loads: instructions with a register destination that pass A tracked (= those in the text); waits: s_waitcnt lines evaluated (= those in
  the text); hazard sites: MFMAs, transcendentals, LDS-DMA, v_readfirstlane, permlane swaps, vector-memory instructions and 16-byte stores
  that pass C held to a rule.  Raised waits: every s_waitcnt count of every kernel raised by one, one at a time; flagged = pass A then
  reports a finding it did not report before.  In the 18 shipped kernels the unflagged ones guard memory, not registers, as expected:
  the LDS-DMA landing waits ahead of a barrier (conv1x1 vmcnt(15 + NDMA) and its + 2 NB arm; c48's and c96's vmcnt(6) / vmcnt(0) at the
  end of an interval; the planar prologue's vmcnt(0), whose youngest operation is an LDS-DMA), lgkmcnt(0) ahead of a barrier or of
  s_endpgm (LDS writes), and in the pixel-major planar families the residual's wait, which earlier waits of the last chunk already cover.
  The ablation builds drop loads or their consumers, which leaves their waits with nothing to guard: most of the other unflagged ones.
  Waived findings, by entry of WAIVERS: planar 1872 + 1872 + 1092 (the residual, 156 reads in each of 12 + 12 + 7 kernels), 62 + 32 + 8
  (timing-only ablations); c48 9 + 3 + 6 + 2; c96 6.  No finding was a real hazard: no generator changed.
  Two things the checker showed on the way, neither a finding: by instruction distance the conv1x1 epilogue's s_nop 15 + s_nop 3 and
  the planar families' "s_nop 15 twice" are not needed (the epilogue starts with accumulators that are a whole k-step / tap of MFMAs old;
  removing them is not flagged in any family), and bottleneck_asm_c48 / _c48_tail end without a vmcnt(0) (waived: stores only).
"""
import os
import re
import subprocess
import sys
import time
from collections import namedtuple

import pytest

import asm_flow

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aquaculture_amd", "csrc")
_ABL = "res1_stamped_abl"
PLANAR = {
    "nb13": ["res0", "res1", "res1_stamped", "res0_w8", "res1_w8", "res1_w8_stamped"] + [f"{_ABL}{a}" for a in (1, 2, 3, 4, 7, 8, 16, 32)],
    "f8nb13": ["res0", "res1", "res1_stamped"] + [f"{_ABL}{a}" for a in (1, 2, 4, 7, 8)],
    "pm13": ["res0", "res1", "res1_stamped"],
    "pm13w20": ["res0", "res1", "res1_stamped"],
    "pm13w40": ["res0", "res1", "res1_stamped"] + [f"{_ABL}{a}" for a in (1, 2, 4, 8, 64, 128, 256)],
    "s2nb13": ["res0", "res0_stamped"] + [f"res0_stamped_abl{a}" for a in (1, 2, 3, 4, 7, 8)],
}
# generator -> (script, its kernels in the order of the file): 4 / 46 / 3 / 2 s_endpgm today
GENERATORS = {
    "conv1x1": ("gen_conv1x1_asm.py", [f"conv1x1_asm_nb{nb}{st}" for nb in (13, 7) for st in ("", "_stamped")]),
    "planar": ("gen_conv3x3_pl_asm.py", [f"conv3x3_pl_asm_{fam}_{v}" for fam, vs in PLANAR.items() for v in vs]),
    "c48": ("gen_bottleneck_asm.py", ["bottleneck_asm_c48", "bottleneck_asm_c48_stamped", "bottleneck_asm_c48_tail"]),
    "c96": ("gen_bottleneck96_asm.py", ["bottleneck_asm_c96", "bottleneck_asm_c96_stamped"]),
}
assert [len(ks) for _, ks in GENERATORS.values()] == [4, 46, 3, 2]
KERNELS = [(g, k) for g, (_, ks) in GENERATORS.items() for k in ks]

# ---- waivers: facts the checker cannot see.  One entry is one site of a generator (one emit loop; its unrolled copies share the entry):
# the kernels it applies to, the rule, the instruction and the finding's detail as patterns, the number of findings it covers in each
# kernel -- exactly that many, or the entry covers none of them -- and the reason.
Waiver = namedtuple("Waiver", "generator kernels rule text detail count reason")
WAIVERS = [
    Waiver("planar", r"_nb13_res1", "read-before-write", r"^v_lshlrev_b32 v2[3-5]\d, 16, v(1[4-9]\d|20\d|21[0-7])$", r"^v(1[4-9]\d|20\d|21[0-7]) ", 156,
           "the residual registers v[140:217] (6 NB, read in both copies of the epilogue) are loaded at the top of the tile's last chunk, "
           "chunk + 1 == nchunks, and the chunk loop is left only behind that chunk, chunk + 1 >= nchunks: a relation between two unknown "
           "scalars"),
    Waiver("planar", r"_pm13(w20|w40)?_res1(?!.*abl256)", "read-before-write", r"^v_lshlrev_b32 v\d+, 16, v(1[0-6]\d|17[0-7])$", r"^v(1[0-6]\d|17[0-7]) ",
           156, "the same for the pixel-major families, whose residual lives in v[100:177]"),
    Waiver("planar", r"_f8nb13_res1", "read-before-write", r"^v_accvgpr_read_b32 v\d+, a\d+$", r"^a(1[5-9]\d|2[0-3]\d) ", 156,
           "the same for the fp8 family, whose residual lives in a[156:233]"),
    Waiver("planar", r"_abl(1|3|7)$", "read-before-write", r"^v_mfma_", r"^[va]\d+ ", {"nb13": {1: 6, 3: 6, 7: 15}, "f8nb13": {1: 3, 7: 8},
           "pm13w40": {1: 6}, "s2nb13": {1: 3, 3: 3, 7: 12}},
           "timing-only ablations with bit 1 (no weight loads; 3 and 7 add 2 and 4), wrong results by design: their MFMAs read registers "
           "that nothing loads"),
    Waiver("planar", r"_abl4$", "read-before-write", r"^v_mfma_", r"^v\d+ ", {"nb13": {4: 9}, "f8nb13": {4: 5}, "pm13w40": {4: 9}, "s2nb13": {4: 9}},
           "timing-only ablation 4 (no B fragment reads), wrong results by design"),
    Waiver("planar", r"_abl256$", "read-before-write", r"^v_permlane16_swap_b32 v2\d\d, v2\d\d$", r"^v2\d\d ", 8,
           "timing-only ablation 256 (no epilogue arithmetic, the stores alone): the store data is never computed"),
    Waiver("c48", r".", "read-before-write", r"^s_mov_b32 s4[678], s4[234]$", r"^s4[234] ", 3,
           "pipeline fill: stage B takes stage D's image and origin even when there is no such tile (d_ok = 0: emit_decode skips "
           "them); every use of b_b, b_y0, b_x0 sits behind b_ok"),
    Waiver("c48", r".", "read-before-write", r"^s_and_b32 s34, s59, s60$", r"^s59 ", 1,
           "rowok0 & rowok1 & c_ok: the row flags are unset until the first phase C, in intervals whose c_ok = 0 zeroes the result"),
    Waiver("c48", r".", "mfma-result", r"^v_pk_mul_f32 v\[220:221\], v\[188:189\], s\[62:63\]$", r"^v188: 15 wait states", 2,
           "phase B, interior tile, block 0 (once per half of the stagger): s_nop 7 plus two MFMAs and five fragment reads put the SiLU's "
           "first read 15 instructions behind the 8-pass MFMA that wrote it, one short of the header's own s_nop 15 = 16; the guide's 12 "
           "states for an 8-pass MFMA are met, and each MFMA in between holds the pipe for its passes, which an instruction count ignores"),
    Waiver("c48", r"c48(_tail)?$", "end-undrained", r"^s_endpgm$", r".", 1,
           "the last tile's output stores (at most six; d_ok = 0 by then, so no LDS-DMA) are in flight at s_endpgm, which the hardware "
           "completes before it frees the wave, as every compiled kernel that ends in a store relies on; the stamped build drains"),
    Waiver("c96", r".", "read-before-write", r"^s_mov_b32 s(59|60|61), s5[123]$", r"^s5[123] ", 3,
           "pipeline fill: the same copy of an undecoded stage D (d_ok = 0) as in the C = 48 kernel"),
]


def _waiver_count(w, kernel):
    if isinstance(w.count, int):
        return w.count
    fam = re.search(r"_asm_([a-z0-9]+)_res", kernel).group(1)
    return w.count.get(fam, {}).get(int(re.search(r"_abl(\d+)$", kernel).group(1)), 0)


def apply_waivers(generator, kernel, findings):
    """(findings no waiver covers, {waiver index: number covered}).  An entry whose pattern matches another number of findings than it
    records covers none of them."""
    left, used = list(findings), {}
    for i, w in enumerate(WAIVERS):
        if w.generator != generator or not re.search(w.kernels, kernel):
            continue
        hit = [f for f in left if f.rule == w.rule and re.search(w.text, f.text) and re.search(w.detail, f.detail)]
        if hit and len(hit) == _waiver_count(w, kernel):
            left = [f for f in left if f not in hit]
            used[i] = len(hit)
    return left, used


# ---- generation, once per generator ----
_cache = {}


def generate(generator):
    if generator not in _cache:
        import tempfile
        env = {k: v for k, v in os.environ.items() if not k.startswith("AQ_GEN_")}
        with tempfile.TemporaryDirectory() as d:
            out = os.path.join(d, generator + ".s")
            subprocess.run([sys.executable, os.path.join(CSRC, GENERATORS[generator][0]), out], check=True, capture_output=True, env=env, cwd=d)
            with open(out) as f:
                text = f.read()
        _cache[generator] = (text, {k.name: k for k in asm_flow.split_kernels(text)}, {})
    return _cache[generator]


def report(generator, kernel):
    _, kernels, reports = generate(generator)
    if kernel not in reports:
        reports[kernel] = asm_flow.check_kernel(kernels[kernel])
    return reports[kernel]


@pytest.fixture(scope="module", params=list(GENERATORS))
def generated(request):
    return request.param, generate(request.param)


def test_kernel_lists(generated):
    generator, (text, kernels, _) = generated
    assert list(kernels) == GENERATORS[generator][1]
    assert len(re.findall(r"^\ts_endpgm", text, re.M)) == len(kernels) == len(re.findall(r"^\t\.amdhsa_kernel ", text, re.M))
    assert all(k.desc.get("next_free_vgpr") and k.desc.get("group_segment_fixed_size") for k in kernels.values())


_LOAD = re.compile(r"^\t(?:(?:global|buffer)_load_dword\w*|ds_read_\w+|ds_bpermute_b32|s_load_dword\w*|s_memtime|s_memrealtime) ([^;\n]*)", re.M)


@pytest.mark.parametrize("generator,kernel", KERNELS)
def test_kernel_has_no_findings(generator, kernel):
    rep = report(generator, kernel)
    left, _ = apply_waivers(generator, kernel, rep.findings)
    assert left == [], "\n".join(f"{f.kernel}:{f.line}: {f.rule}: {f.text}   ({f.detail})" for f in left[:20])
    # not vacuous: every load with a register destination was tracked, every wait evaluated (a block no path reaches would miss here),
    # every class of hazard site was met
    text = generate(generator)[1][kernel].text
    loads = [m.group(1) for m in _LOAD.finditer(text) if not m.group(1).rstrip().endswith(" lds")]
    assert rep.loads == len(loads) > 0
    assert rep.waits == len(re.findall(r"^\ts_waitcnt ", text, re.M)) > 0
    assert rep.instructions == len(re.findall(r"^\t[a-z]", text, re.M))
    assert rep.sites["m0-dma"] == len(re.findall(r"^\t(?:global_load_lds_\w+ |buffer_load_\w+ [^;\n]* lds\b)", text, re.M))
    assert rep.sites["valu-readfirstlane"] == len(re.findall(r"^\tv_readfirstlane_b32 ", text, re.M)) > 0
    assert rep.sites["valu-permlane"] == len(re.findall(r"^\tv_permlane\d+_swap_b32 ", text, re.M))
    assert rep.sites["mfma-result"] == len(re.findall(r"^\tv_mfma_", text, re.M))
    assert rep.sites["trans-result"] == len(re.findall(r"^\tv_(?:exp|rcp)_f32 ", text, re.M))


def test_every_waiver_is_used():
    used = set()
    for generator, kernel in KERNELS:
        used |= set(apply_waivers(generator, kernel, report(generator, kernel).findings)[1])
    assert used == set(range(len(WAIVERS)))


# ---- mutations of the real text: (generator, kernel, pattern, replacement, rule that must fire) ----
def _trans_next(m):
    """The multiply behind the last v_rcp of a SiLU batch takes that v_rcp's result instead of the batch's first."""
    t = int(m.group(2))
    return f"{m.group(1)}v[{t - 1}:{t}]"


_SILU_END = r"(v_rcp_f32 v(\d+), v\2\n\tv_pk_mul_f32 v\[\d+:\d+\], v\[\d+:\d+\], )v\[\d+:\d+\]"
_M0_NOP = (r"(\ts_(?:add_u32|mov_b32) m0, [^\n]*\n)\ts_nop 0[^\n]*\n", r"\1")
_RFL_NOP = (r"\ts_nop 1[^\n]*\n(\tv_readfirstlane_b32 )", r"\1")
_LOAD_CLOBBER = (r"(\tglobal_load_dwordx[24] v\[(\d+):\d+\], [^\n]*\n)", r"\1\tv_mov_b32 v\2, 0\n")
# a VALU-written scalar as the base of the next global load (the generators compute such bases on the SALU)
_SGPR_VMEM = (r"(\tglobal_load_dwordx[24] [av]\[\d+:\d+\], v\d+, s\[(\d+):\d+\][^\n]*\n)", r"\tv_readfirstlane_b32 s\2, v0\n\1")
MUTATIONS = [
    # gen_conv1x1_asm.py
    ("conv1x1", "conv1x1_asm_nb13", r"s_waitcnt vmcnt\(6\)", "s_waitcnt vmcnt(7)", "read-pending"),           # emit_body: k-step 0's weights
    ("conv1x1", "conv1x1_asm_nb13", r"s_waitcnt vmcnt\(32\)", "s_waitcnt vmcnt(33)", "read-pending"),         # ... its arm behind an epilogue
    ("conv1x1", "conv1x1_asm_nb7", r"s_waitcnt vmcnt\(9\)", "s_waitcnt vmcnt(10)", "read-pending"),           # k-steps 1, 2: 6 + NDMA
    ("conv1x1", "conv1x1_asm_nb13", r"s_waitcnt lgkmcnt\(4\)", "s_waitcnt lgkmcnt(5)", "read-pending"),       # lgkmcnt(PD)
    # epilogue: its first block is a whole k-step of MFMAs old, so shortening s_nop 15 + s_nop 3 alone breaks nothing the checker (or the
    # hardware) could see; without them and with the LAST accumulator tile as the first SiLU input it is 6 states, not 16
    ("conv1x1", "conv1x1_asm_nb13", r"\ts_nop 15[^\n]*\n\ts_nop 3\n((?:\ts_[^\n]*\n){6}\tv_pk_mul_f32 v\[\d+:\d+\], )v\[4:5\]", r"\1v[158:159]",
     "mfma-result"),
    ("conv1x1", "conv1x1_asm_nb7", *_M0_NOP, "m0-dma"),
    ("conv1x1", "conv1x1_asm_nb13", *_RFL_NOP, "valu-readfirstlane"),
    ("conv1x1", "conv1x1_asm_nb13", r"(\.Lend_conv1x1_asm_nb13:\n)\ts_waitcnt vmcnt\(0\)[^\n]*\n", r"\1", "end-undrained"),
    ("conv1x1", "conv1x1_asm_nb13", r"(v_mfma_f32_16x16x32_bf16 )v\[4:7\](, [^\n]*, )v\[4:7\]", r"\1v[248:251]\2v[248:251]", "vgpr-budget"),
    ("conv1x1", "conv1x1_asm_nb7", r"\tv_and_b32 v\d+, 15, v\d+[^\n]*\n", "", "read-before-write"),           # p15 never computed
    ("conv1x1", "conv1x1_asm_nb13", r"(ds_read_b128 v\[\d+:\d+\], v\d+ offset:)\d+", r"\g<1>125952", "lds-offset"),
    ("conv1x1", "conv1x1_asm_nb13", _SILU_END, _trans_next, "trans-result"),
    ("conv1x1", "conv1x1_asm_nb13", r"(\tbuffer_load_dwordx4 v\[\d+:\d+\], v\d+, s\[\d+:\d+\], (s\d+) offen)", r"\tv_readfirstlane_b32 \2, v0\n\1",
     "valu-sgpr-vmem"),
    ("conv1x1", "conv1x1_asm_nb13", r"(\tbuffer_store_dwordx4 v\[(\d+):\d+\], [^\n]*\n)", r"\1\tv_mov_b32 v\2, 0\n", "store16-data"),
    ("conv1x1", "conv1x1_asm_nb13", r"(\tbuffer_load_dwordx4 v\[(\d+):\d+\], v\d+, [^\n]*\n)", r"\1\tv_mov_b32 v\2, 0\n", "write-pending"),
    ("conv1x1", "conv1x1_asm_nb13_stamped", r"v_lshl_add_u32 ", "v_lshl_add_u64 ", "unclassified"),
    ("conv1x1", "conv1x1_asm_nb7", r"s_mov_b32 s\d+, 0xbfb8aa3b", "s_mov_b32 s100, 0xbfb8aa3b", "sgpr-budget"),
    # gen_conv3x3_pl_asm.py
    ("planar", "conv3x3_pl_asm_nb13_res1", r"s_waitcnt vmcnt\(9\)", "s_waitcnt vmcnt(10)", "read-pending"),   # weights of tap 0, loads 0 .. 2
    ("planar", "conv3x3_pl_asm_nb13_res1", r"s_waitcnt vmcnt\(48\)", "s_waitcnt vmcnt(49)", "read-pending"),  # ... behind an epilogue: + 3 NB
    # the residual's wait has one to spare (its youngest load has 13 younger, the wait says 12), and in the pixel-major families the
    # residual has landed under earlier waits: there raising this one is not flagged at all
    ("planar", "conv3x3_pl_asm_nb13_res1", r"s_waitcnt vmcnt\(12\)([^\n]*the residual)", r"s_waitcnt vmcnt(14)\1", "read-pending"),
    ("planar", "conv3x3_pl_asm_f8nb13_res0", r"s_waitcnt lgkmcnt\(6\)", "s_waitcnt lgkmcnt(7)", "read-pending"),
    # "s_nop 15 twice before the epilogue": the epilogue starts with the accumulators a whole tap of MFMAs old and the loop's scalar tail
    # stands in between, so by instruction distance the two are not needed (removing them is not flagged in any family, nor is reading
    # the LAST tile first: 18 states in nb13, 16 needed).  A read of the last tile placed right behind the stream's last MFMA is flagged.
    ("planar", "conv3x3_pl_asm_s2nb13_res0", r"(\tv_mfma_f32_16x16x32_bf16 a\[152:155\], [^\n]*\n)(\ts_add_u32 s62, s51, 1\n)",
     r"\1\tv_accvgpr_read_b32 v180, a152\n\2", "mfma-result"),
    ("planar", "conv3x3_pl_asm_nb13_res0", *_M0_NOP, "m0-dma"),
    ("planar", "conv3x3_pl_asm_pm13_res0", *_RFL_NOP, "valu-readfirstlane"),
    ("planar", "conv3x3_pl_asm_pm13_res0", r"(\tv_permlane16_swap_b32 (v\d+), v\d+\n)", r"\tv_mov_b32 \2, \2\n\1", "valu-permlane"),
    ("planar", "conv3x3_pl_asm_nb13_res0", r"(\.Lend_conv3x3_pl_asm_nb13_res0:\n)\ts_waitcnt vmcnt\(0\)[^\n]*\n", r"\1", "end-undrained"),
    ("planar", "conv3x3_pl_asm_nb13_res0", r"(v_mfma_f32_16x16x32_bf16 )a\[152:155\](, [^\n]*, )a\[152:155\]", r"\1a[256:259]\2a[256:259]", "agpr-budget"),
    ("planar", "conv3x3_pl_asm_f8nb13_res1", r"(ds_read_b128 v\[\d+:\d+\], v\d+ offset:)0\n", r"\g<1>163840\n", "lds-offset"),
    ("planar", "conv3x3_pl_asm_pm13w20_res1", *_LOAD_CLOBBER, "write-pending"),
    ("planar", "conv3x3_pl_asm_nb13_res0_w8", r"v_cvt_pk_f32_fp8_e32 ", "v_cvt_pk_f32_bf8_e32 ", "unclassified"),
    ("planar", "conv3x3_pl_asm_pm13_res0", r"(\tglobal_store_dwordx4 v\d+, v\[(\d+):\d+\], [^\n]*\n)", r"\1\tv_mov_b32 v\2, 0\n", "store16-data"),
    ("planar", "conv3x3_pl_asm_nb13_res0", r"\tv_and_b32 v\d+, 15, v\d+[^\n]*\n", "", "read-before-write"),
    ("planar", "conv3x3_pl_asm_nb13_res0", r"ds_read_b128 v\[84:87\]", "ds_read_b128 v[256:259]", "vgpr-budget"),
    ("planar", "conv3x3_pl_asm_s2nb13_res0", r"s_mov_b32 s\d+, 0xbfb8aa3b", "s_mov_b32 s100, 0xbfb8aa3b", "sgpr-budget"),
    # without a residual two s_nop 0 stand between the last v_rcp and the multiplies; the first multiply takes the batch's first result
    ("planar", "conv3x3_pl_asm_nb13_res0", r"(v_rcp_f32 v(\d+), v\2\n)\ts_nop 0\n\ts_nop 0\n(\tv_pk_mul_f32 v\[\d+:\d+\], v\[\d+:\d+\], )v\[\d+:\d+\]",
     lambda m: f"{m.group(1)}{m.group(3)}v[{int(m.group(2)) - 1}:{m.group(2)}]", "trans-result"),
    ("planar", "conv3x3_pl_asm_pm13w40_res0", *_SGPR_VMEM, "valu-sgpr-vmem"),
    # gen_bottleneck_asm.py
    ("c48", "bottleneck_asm_c48", r"s_waitcnt vmcnt\(4\)", "s_waitcnt vmcnt(5)", "read-pending"),             # shortcut values, four LDS-DMA behind them
    ("c48", "bottleneck_asm_c48", r"s_waitcnt lgkmcnt\(3\)", "s_waitcnt lgkmcnt(4)", "read-pending"),         # phase B: block 1's fragments and b1
    ("c48", "bottleneck_asm_c48_tail", r"s_waitcnt vmcnt\(0\)([^\n]*the cv2 values)", r"s_waitcnt vmcnt(1)\1", "read-pending"),
    ("c48", "bottleneck_asm_c48", r"s_nop 15([^\n]*\n\ts_cmp_eq_u32 s\d+, 0\n)", r"s_nop 0\1", "mfma-result"),  # phase C: the s_nop 15 ahead of the epilogue
    ("c48", "bottleneck_asm_c48", *_M0_NOP, "m0-dma"),
    ("c48", "bottleneck_asm_c48_stamped", *_RFL_NOP, "valu-readfirstlane"),
    ("c48", "bottleneck_asm_c48_tail", r"(\tv_permlane16_swap_b32 (v\d+), v\d+\n)", r"\tv_mov_b32 \2, \2\n\1", "valu-permlane"),
    ("c48", "bottleneck_asm_c48_tail", r"(\tglobal_store_dwordx4 v\d+, v\[(\d+):\d+\], [^\n]*\n)", r"\1\tv_mov_b32 v\2, 0\n", "store16-data"),
    ("c48", "bottleneck_asm_c48_stamped", r"(\tglobal_store_dwordx2 [^\n]*\n)\ts_waitcnt vmcnt\(0\)\n(\ts_endpgm)", r"\1\2", "end-undrained"),
    ("c48", "bottleneck_asm_c48", r"\tv_and_b32 v\d+, 15, v\d+[^\n]*\n", "", "read-before-write"),            # l15 never computed
    ("c48", "bottleneck_asm_c48", r"(ds_read_b128 v\[\d+:\d+\], v\d+ offset:)1024\n", r"\g<1>137728\n", "lds-offset"),
    ("c48", "bottleneck_asm_c48", r"s_mov_b32 s62, 0xbfb8aa3b", "s_mov_b32 s100, 0xbfb8aa3b", "sgpr-budget"),
    ("c48", "bottleneck_asm_c48", _SILU_END, _trans_next, "trans-result"),
    ("c48", "bottleneck_asm_c48", *_LOAD_CLOBBER, "write-pending"),
    ("c48", "bottleneck_asm_c48", r"v_mul_u32_u24 ", "v_mul_i32_i24 ", "unclassified"),
    ("c48", "bottleneck_asm_c48", r"(v_mfma_f32_16x16x32_bf16 )v\[188:191\](, [^\n]*, )v\[188:191\]", r"\1v[256:259]\2v[256:259]", "vgpr-budget"),
    ("c48", "bottleneck_asm_c48", *_SGPR_VMEM, "valu-sgpr-vmem"),
    # gen_bottleneck96_asm.py
    ("c96", "bottleneck_asm_c96", r"s_waitcnt vmcnt\(0\)([^\n]*shortcut)", r"s_waitcnt vmcnt(1)\1", "read-pending"),
    ("c96", "bottleneck_asm_c96", r"s_waitcnt lgkmcnt\(0\)\n(\tv_mfma)", r"s_waitcnt lgkmcnt(1)\n\1", "read-pending"),
    ("c96", "bottleneck_asm_c96", r"s_nop 15([^\n]*MFMA result -> VALU read\n)", r"s_nop 1\1", "mfma-result"),
    ("c96", "bottleneck_asm_c96", *_M0_NOP, "m0-dma"),
    ("c96", "bottleneck_asm_c96_stamped", *_RFL_NOP, "valu-readfirstlane"),
    ("c96", "bottleneck_asm_c96", r"(\.Lend_bottleneck_asm_c96:\n)\ts_waitcnt vmcnt\(0\)[^\n]*\n", r"\1", "end-undrained"),
    ("c96", "bottleneck_asm_c96", r"buffer_load_dwordx4 a\[252:255\]", "buffer_load_dwordx4 a[256:259]", "agpr-budget"),
    ("c96", "bottleneck_asm_c96", r"(v_mfma_f32_16x16x32_bf16 )v\[108:111\](, [^\n]*, )v\[108:111\]", r"\1v[252:255]\2v[252:255]", "vgpr-budget"),
    ("c96", "bottleneck_asm_c96", r"\tv_and_b32 v\d+, 15, v\d+[^\n]*\n", "", "read-before-write"),
    ("c96", "bottleneck_asm_c96", _SILU_END, _trans_next, "trans-result"),
    ("c96", "bottleneck_asm_c96", *_LOAD_CLOBBER, "write-pending"),
    ("c96", "bottleneck_asm_c96", r"(\tbuffer_store_dwordx4 v\[(\d+):\d+\], [^\n]*\n)", r"\1\tv_mov_b32 v\2, 0\n", "store16-data"),
    ("c96", "bottleneck_asm_c96", r"v_pk_mul_f32 ", "v_pk_fma_f32 ", "unclassified"),
    ("c96", "bottleneck_asm_c96", r"s_mov_b32 s\d+, 0xbfb8aa3b", "s_mov_b32 s102, 0xbfb8aa3b", "sgpr-budget"),
    ("c96", "bottleneck_asm_c96", r"(ds_read_b128 v\[\d+:\d+\], v\d+ offset:)\d+", r"\g<1>163840", "lds-offset"),
    ("c96", "bottleneck_asm_c96", r"(\tbuffer_load_dwordx4 [av]\[\d+:\d+\], v\d+, s\[\d+:\d+\], (s\d+) offen)", r"\tv_readfirstlane_b32 \2, v0\n\1", "valu-sgpr-vmem"),
]


def mutate(generator, kernel, pattern, repl):
    """The generated file with one edit inside `kernel` (the pattern's first match there)."""
    text = generate(generator)[0]
    start = text.index(f"\n{kernel}:\n") + 1
    end = text.index("\ts_endpgm", start) + len("\ts_endpgm")
    body, n = re.subn(pattern, repl, text[start:end], count=1)
    assert n == 1, f"the pattern {pattern!r} does not occur in {kernel}"
    return text[:start] + body + text[end:]


@pytest.mark.parametrize("generator,kernel,pattern,repl,rule", MUTATIONS, ids=[f"{m[1]}-{m[4]}-{i}" for i, m in enumerate(MUTATIONS)])
def test_mutation_is_flagged(generator, kernel, pattern, repl, rule):
    base = generate(generator)[1]
    mutated = {k.name: k for k in asm_flow.split_kernels(mutate(generator, kernel, pattern, repl))}
    assert list(mutated) == list(base)
    for name, k in mutated.items():                      # the others are untouched: their text, hence their (clean) reports, stand
        assert (k.text == base[name].text) == (name != kernel)
    before = {(f.rule, f.text, f.detail) for f in report(generator, kernel).findings}
    only = "A" if rule in ("read-pending", "write-pending", "end-undrained") else "C" if rule in asm_flow.HAZARDS else "B"    # the rule's pass
    left, _ = apply_waivers(generator, kernel, asm_flow.check_kernel(mutated[kernel], passes=only).findings)
    new = [f for f in left if (f.rule, f.text, f.detail) not in before]
    assert rule in {f.rule for f in new}, sorted({f.rule for f in new})


# ---- the recorded table ----
def _raised(args):
    """How many of a kernel's waits, each raised by one on its own, does pass A flag?"""
    generator, name = args
    k = generate(generator)[1][name]
    blocks, succs, _ = asm_flow.expand_cfg(k)
    flagged = {"vmcnt": [0, 0], "lgkmcnt": [0, 0]}
    before = set()
    asm_flow._pass_a(k, blocks, succs, asm_flow.KernelReport(name), lambda ins, rule, detail: before.add((ins.line, rule)))
    for x in k.ins:
        if x.cls != asm_flow.WAIT:
            continue
        for field in list(x.imm):
            hits = []
            x.imm[field] += 1
            asm_flow._pass_a(k, blocks, succs, asm_flow.KernelReport(name), lambda ins, rule, detail: hits.append((ins.line, rule)))
            x.imm[field] -= 1
            flagged[field][0] += bool(set(hits) - before)
            flagged[field][1] += 1
    return generator, name, flagged


def main():
    from multiprocessing import Pool
    t0 = time.time()
    rows = {}
    for generator, (_, names) in GENERATORS.items():
        tot = dict(kernels=0, ins=0, loads=0, waits=0, sites=0, waived=0)
        for name in names:
            rep = report(generator, name)
            left, used = apply_waivers(generator, name, rep.findings)
            assert not left, left[:3]
            for key, v in (("kernels", 1), ("ins", rep.instructions), ("loads", rep.loads), ("waits", rep.waits), ("sites", sum(rep.sites.values())),
                           ("waived", sum(used.values()))):
                tot[key] += v
        rows[generator] = tot
    print(f"checked in {time.time() - t0:.0f} s")
    shipped = KERNELS
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        raised = pool.map(_raised, shipped, chunksize=1)
    print("generator  kernels  instructions   loads   waits  hazard sites  waived findings   raised vmcnt flagged   raised lgkmcnt flagged")
    for generator, tot in rows.items():
        vm = [sum(r[2]["vmcnt"][i] for r in raised if r[0] == generator) for i in (0, 1)]
        lg = [sum(r[2]["lgkmcnt"][i] for r in raised if r[0] == generator) for i in (0, 1)]
        print(f"{generator:9s}  {tot['kernels']:7d}  {tot['ins']:12d}  {tot['loads']:6d}  {tot['waits']:6d}  {tot['sites']:12d}  {tot['waived']:15d}"
              f"   {vm[0]:6d} of {vm[1]:5d}         {lg[0]:6d} of {lg[1]:5d}")
    print(f"(raised waits: all {len(shipped)} kernels)   total {time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
