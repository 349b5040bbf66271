"""Build-time check of the C3 tail kernel (gen_bottleneck_asm.py TAIL, bottleneck_asm_c48_tail) -- no GPU needed.

  * the shipped C = 48 kernel is generated exactly as without the tail option (the tail is a separate kernel of the same code object);
  * per phase-C copy: the 36 MFMAs of cv3, six 16-byte output stores and no 8-byte ones, four cv2 loads, and the tile-end wait that
    lets exactly the six stores stay in flight (vmcnt is in order: a larger count would let the next x patch's LDS-DMA through);
  * the hazards the assembler does not pad: no VALU write of an operand within two instructions ahead of a v_permlane*_swap, no VALU
    write of a 16-byte store's data registers in the two instructions behind it (gfx940+)."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "aquaculture_amd", "csrc", "gen_bottleneck_asm.py")


def _regs(text):
    r = set()
    for m in re.finditer(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]", text):
        r |= {int(m.group(1))} if m.group(1) else set(range(int(m.group(2)), int(m.group(3)) + 1))
    return r


def _generate(tmp_path):
    out = tmp_path / "btl.s"
    env = {k: v for k, v in os.environ.items() if not k.startswith("AQ_GEN_")}
    subprocess.run([sys.executable, GEN, str(out)], check=True, capture_output=True, env=env)
    return out.read_text()


def _body(text, name):
    return [l.split(";")[0].strip() for l in text.split(f"\n{name}:\n", 1)[1].split("s_endpgm", 1)[0].split("\n") if l.startswith("\t")]


def test_tail_kernel_memory_operations_and_waits(tmp_path):
    text = _generate(tmp_path)
    base, tail = _body(text, "bottleneck_asm_c48"), _body(text, "bottleneck_asm_c48_tail")
    mf = lambda ins: sum(l.startswith("v_mfma") for l in ins)
    assert mf(tail) == mf(base) + 2 * 36                          # phase C is emitted twice (the two halves of the stagger)
    stores = [l for l in tail if l.startswith("global_store")]
    assert len(stores) == 2 * 6 and all(l.startswith("global_store_dwordx4") for l in stores)
    assert sum(l.startswith("global_load_dwordx4") and "offset:32" in l for l in tail) == 2 * 2      # cv2 channels 16-47, two rows
    # the tile-end waits before the barrier: the six output stores may stay in flight, nothing else
    assert re.findall(r"s_waitcnt vmcnt\((\d+)\)", "\n".join(base)).count("6") == 1
    assert re.findall(r"s_waitcnt vmcnt\((\d+)\)", "\n".join(tail)).count("6") == 1
    assert "group_segment_fixed_size 156416" in text and "kernarg_size 112" in text


def test_tail_kernel_hazards(tmp_path):
    ins = _body(_generate(tmp_path), "bottleneck_asm_c48_tail")
    n_perm = n_st = 0
    for i, l in enumerate(ins):
        if l.startswith(("v_permlane16_swap", "v_permlane32_swap")):
            n_perm += 1
            ops = _regs(l)
            for back in (1, 2):
                dst = re.match(r"v_\S+ (v\d+|v\[\d+:\d+\])", ins[i - back])
                assert not dst or not (_regs(dst.group(1)) & ops), f"'{ins[i - back]}' writes an operand of '{l}' {back} instruction(s) ahead"
        if l.startswith("global_store_dwordx4"):
            n_st += 1
            data = _regs(l.split(",")[1])
            for ahead in (1, 2):
                nxt = re.match(r"v_\S+ (v\d+|v\[\d+:\d+\])", ins[i + ahead])
                assert not nxt or not (_regs(nxt.group(1)) & data), f"'{ins[i + ahead]}' rewrites the data of '{l}'"
    assert n_perm == 2 * (16 + 3 * 4) and n_st == 12


def test_shipped_kernel_is_unchanged_by_the_tail_option(tmp_path):
    """The generator emits the shipped kernel and its stamped build before the tail kernel, with the same text as a generator run that
    stops before the tail (the tail only adds a kernel)."""
    text = _generate(tmp_path)
    head, _ = text.split("\t.globl\tbottleneck_asm_c48_tail", 1)
    assert "bottleneck_asm_c48:" in head and "bottleneck_asm_c48_stamped:" in head
    assert "s88" not in "\n".join(_body(text, "bottleneck_asm_c48"))            # the tail's scalars (stamp accumulators) stay out of it
