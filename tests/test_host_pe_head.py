"""The head of the fused MLP kernels -- everything ahead of a wave's first MFMA -- as the SHIPPED assembly shows it
(build/nerf_fwd_x16.s, kept by the Makefile next to the object).  While the eight waves of a workgroup sit in their heads
nothing else is on the CU's matrix pipe, so the positional encoder (csrc/x16_core.h: pe_encode) handles every (octave, axis)
once: 15 pairs = 30 v_sin_f32 per lane, no channel index decoded at run time, no sine evaluated to be thrown away.  The
per-channel form it replaced had 32 sines and 1 326 / 1 303 / 1 303 vector-ALU instructions in the head (bf16 / fp16 inference,
training forward); the cap here is a condition, the counts themselves are in docs/tuning_log.md."""
import glob
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kernel label prefix -> scratch bytes allowed.  The training forward sits at 256 registers and its budget is the 16 bytes
# csrc/nerf_fwd_x16.hip documents for it (one or two dwords that cross the whole stream: 8 bytes with the per-channel encoder,
# 12 with this one -- the sampler's (z_lo, z_hi) pair now reaches the stream whole and is spilled whole)
KERNELS = {
    "_Z19nerf_fwd_x16_kernelILi1ELi8EE": 0,     # bf16
    "_Z19nerf_fwd_x16_kernelILi2ELi8EE": 0,     # fp16
    "_Z25nerf_fwd_x16_train_kernelILi8EE": 16,
}
VALU_CAP = 900


def _assembly():
    files = sorted(glob.glob(os.path.join(REPO, "nerf-3dtalker-code_amd", "build", "nerf_fwd_x16.s")))
    if not files:
        pytest.skip("no device assembly under nerf-3dtalker-code_amd/build (built artefacts are git-ignored and no hipcc built them here)")
    return open(files[0]).read()


def _kernel(text, prefix):
    """(instructions of the kernel whose label starts with prefix, its .amdhsa descriptor)"""
    labels = [m.group(1) for m in re.finditer(r"^(_Z\S+):", text, re.M) if m.group(1).startswith(prefix)]
    assert len(labels) == 1, (prefix, labels)
    body = text[text.index("\n" + labels[0] + ":"):]
    body = body[:body.index("s_endpgm")]
    code = [c for c in (line.split(";")[0].strip() for line in body.split("\n")[2:]) if c and not c.startswith(".") and not c.endswith(":")]
    desc = text[text.index(".amdhsa_kernel " + labels[0]):]
    return code, desc[:desc.index(".end_amdhsa_kernel")]


def head_counts(text, prefix):
    """{'insts', 'valu', 'salu', 'sin'} of the instructions before the kernel's first MFMA"""
    code, _ = _kernel(text, prefix)
    first = next(i for i, c in enumerate(code) if c.startswith("v_mfma"))
    head = code[:first]
    return {"insts": len(head), "valu": sum(c.startswith("v_") for c in head),
            "salu": sum(c.startswith("s_") for c in head),
            "sin": sum(c.startswith("v_sin_f32") for c in head)}


@pytest.mark.parametrize("prefix", sorted(KERNELS))
def test_head_has_thirty_sines_and_fewer_than_900_valu(prefix):
    n = head_counts(_assembly(), prefix)
    print("%s: head %d instructions, %d vector-ALU, %d scalar, %d v_sin_f32" % (prefix, n["insts"], n["valu"], n["salu"], n["sin"]))
    assert n["sin"] == 30          # 5 octaves x 3 axes x (sine, cosine) per lane half
    assert n["valu"] < VALU_CAP


@pytest.mark.parametrize("prefix", sorted(KERNELS))
def test_encoder_is_straight_line_code(prefix):
    """From the first phase reduction to the last LDS store of the scatter the lane mask is never narrowed and nothing branches:
    the raw coordinates and the zero channel ride along by select, the per-half destinations are selects of two constants."""
    code, _ = _kernel(_assembly(), prefix)
    first = next(i for i, c in enumerate(code) if c.startswith("v_mfma"))
    head = code[:first]
    start = next(i for i, c in enumerate(head) if c.startswith("v_fract_f32"))
    end = max(i for i, c in enumerate(head) if c.startswith(("v_sin_f32", "ds_write_b16", "ds_write_b32")))
    span = head[start:end + 1]
    assert sum(c.startswith("v_sin_f32") for c in span) == 30
    assert sum(c.startswith("ds_write_b32") for c in span) == 15 and sum(c.startswith("ds_write_b16") for c in span) == 3
    assert not [c for c in span if re.match(r"s_\w+_saveexec_b64|s_cbranch|s_branch", c) or re.search(r"\bexec\b", c)]


@pytest.mark.parametrize("prefix", sorted(KERNELS))
def test_registers_and_scratch(prefix):
    _, desc = _kernel(_assembly(), prefix)
    vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc).group(1))
    scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc).group(1))
    assert vgpr <= 256             # two waves per SIMD
    assert scratch <= KERNELS[prefix]
