"""The weight stream's issue schedule as the SHIPPED assembly shows it (build/nerf_fwd_x16.s, kept by the Makefile next to
the object; csrc/x16_core.h: X16Issue, WeightStream).  Per fused MLP kernel: every chunk of the stream is staged by the same
number of LDS-DMA instructions per wave, the prologue's NBUF - 1 chunks before the first barrier, then one chunk between each
pair of consecutive rendezvous barriers while chunks remain, and nothing in the stream's tail; a kernel on a spread schedule
has matrix instructions between the pieces of a period and addresses every piece from a scalar base; and the register /
scratch figures docs/tuning_log.md records."""
import glob
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

X16_CH, X16_NCHUNK, NBUF, WAVES = 24, 95, 3, 8      # csrc/x16_core.h; eight waves per workgroup in all three kernels
PPW = X16_CH // WAVES                              # pieces a wave stages per chunk

# kernel label prefix -> (on a spread schedule, inference kernel)
KERNELS = {
    "_Z19nerf_fwd_x16_kernelILi1ELi8EE": (True, True),    # bf16
    "_Z19nerf_fwd_x16_kernelILi2ELi8EE": (True, True),    # fp16
    "_Z25nerf_fwd_x16_train_kernelILi8EE": (False, False),
}


def _kernels():
    """label -> (events, text): events is the kernel's instruction stream reduced to D (LDS-DMA piece), B (barrier), M (MFMA)"""
    files = sorted(glob.glob(os.path.join(REPO, "nerf-3dtalker-code_amd", "build", "nerf_fwd_x16.s")))
    if not files:
        pytest.skip("no device assembly under nerf-3dtalker-code_amd/build (built artefacts are git-ignored and no hipcc built them here)")
    text = open(files[0]).read()
    label = re.compile(r"^(_Z\S+):")
    out, cur = {}, None
    for line in text.split("\n"):
        m = label.match(line)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        code = line.split(";")[0].strip()
        if cur is None or not code or code.startswith("."):
            continue
        if code.startswith("global_load_lds_dwordx4"):
            out[cur].append("D")
        elif re.match(r"s_barrier\b", code):
            out[cur].append("B")
        elif code.startswith("v_mfma"):
            out[cur].append("M")
    return {k: "".join(v) for k, v in out.items()}, text


def _find(kernels, prefix):
    hit = [k for k in kernels if k.startswith(prefix)]
    assert len(hit) == 1, (prefix, hit)
    return hit[0]


@pytest.mark.parametrize("prefix", sorted(KERNELS))
def test_every_chunk_is_issued_once_between_its_two_rendezvous(prefix):
    kernels, _ = _kernels()
    ev = kernels[_find(kernels, prefix)]
    assert ev.count("D") == X16_NCHUNK * PPW == 285
    assert ev.count("B") == X16_NCHUNK + 1          # the prologue's barrier and one rendezvous per chunk
    periods = ev.split("B")
    dma = [p.count("D") for p in periods]
    assert dma[0] == (NBUF - 1) * PPW               # the prologue stages NBUF - 1 chunks whole
    assert dma[1] == 0                              # (they are awaited by the prologue's barrier; rendezvous 0 stages the next)
    staged = X16_NCHUNK - (NBUF - 1)                # chunks staged behind a rendezvous: one per period, from rendezvous 0 on
    assert dma[2:2 + staged] == [PPW] * staged
    assert dma[2 + staged:] == [0] * (NBUF - 1)     # the tail issues nothing
    spread = KERNELS[prefix][0]
    gaps = [len(seg) for p in periods[2:2 + staged] for seg in p.split("D")[1:-1]]
    assert len(gaps) == staged * (PPW - 1)
    if spread:
        # the pieces of a period sit between the MFMAs, not back to back behind the barrier
        assert min(gaps) >= 1, "two LDS-DMA pieces of a period with no MFMA between them"


@pytest.mark.parametrize("prefix", sorted(KERNELS))
def test_registers_and_scratch(prefix):
    kernels, text = _kernels()
    name = _find(kernels, prefix)
    desc = text[text.index(".amdhsa_kernel " + name):]
    desc = desc[:desc.index(".end_amdhsa_kernel")]
    vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc).group(1))
    scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc).group(1))
    assert vgpr <= 256                              # two waves per SIMD
    if KERNELS[prefix][1]:
        assert scratch == 0


@pytest.mark.parametrize("prefix", sorted(k for k, v in KERNELS.items() if v[0]))
def test_spread_pieces_are_addressed_from_a_scalar_base(prefix):
    """`global_load_lds_dwordx4 vN, s[a:b]`: one 32-bit lane offset and a scalar base, no register pair and no 64-bit vector
    add per piece.  The builtin gives that form only while WeightStream::issue_piece keeps the base and the offset opaque; a
    compiler that folds them into a per-lane pointer again fails here."""
    _, text = _kernels()
    body = text[text.index("\n" + prefix):]
    body = body[:body.index(".end_amdhsa_kernel")]
    code = [c for c in (line.split(";")[0].strip() for line in body.split("\n")) if c and not c.startswith(".") and not c.endswith(":")]
    at = [i for i, c in enumerate(code) if c.startswith("global_load_lds_dwordx4")]
    assert len(at) == X16_NCHUNK * PPW
    for i in at:
        assert re.fullmatch(r"global_load_lds_dwordx4 v\d+, s\[\d+:\d+\]", code[i]), code[i]
        assert not any(c.startswith("v_lshl_add_u64") for c in code[max(0, i - 3):i]), code[max(0, i - 3):i + 1]
