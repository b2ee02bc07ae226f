"""GPU: the GREAT training head's forward (hip_ops.varmisuse_head, csrc/bl_varmisuse_head.hip) against bits recorded on an MI355X
before its row arithmetic moved to csrc/bl_varmisuse_rows.h (tests/golden/varmisuse_train_logits.npz: masked logits and
[loss, number of buggy samples] as int32 bit patterns, one entry per case, and a SHA-256 of each case's fp32 input so that a
drift of the input generator is told apart from a drift of the kernel).  Every width class of the row kernel is covered:
1, 2 (one with a partly filled last chunk), 3 and 4 float4 chunks per lane."""
import hashlib
import os

import numpy as np
import pytest
import torch

from tests.test_great_varmisuse_gpu import _head_case

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "varmisuse_train_logits.npz")
CASES = [
    dict(D=64, B=3, L=23, seed=0, full_lengths=True),
    dict(D=128, B=4, L=37, seed=1, no_bug=True),
    dict(D=260, B=3, L=11, seed=6),
    dict(D=512, B=5, L=64, seed=2, ties=True),
    dict(D=768, B=2, L=9, seed=7),
    dict(D=1024, B=2, L=8, seed=5),
]


def head_forward_bits(case):
    """-> (SHA-256 of the fp32 x, logits bits int32 [B * L, 2], [loss, number of buggy samples] bits int32 [2])."""
    from buglab.models import hip_ops

    x, ln_g, ln_b, W, bias, lens_att, err, cand, tgt = _head_case(**case)
    f = lambda t: t.float().cuda()
    x32 = x.float()
    stats = torch.zeros(hip_ops.VARMISUSE_STATS, dtype=torch.float64, device="cuda")
    with torch.no_grad():
        loss, logits, nb = hip_ops.varmisuse_head(x32.cuda(), f(ln_g), f(ln_b), f(W), f(bias), lens_att.cuda(), err.cuda(), cand.cuda(),
                                                  tgt.cuda(), stats)
    sha = hashlib.sha256(x32.numpy().tobytes()).hexdigest()
    return sha, logits.cpu().view(torch.int32).numpy(), torch.stack([loss, nb]).cpu().view(torch.int32).numpy()


@pytest.mark.parametrize("k", range(len(CASES)), ids=lambda k: f"D{CASES[k]['D']}")
def test_training_forward_bits_are_the_recorded_ones(k):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    z = np.load(GOLD)
    sha, logits, loss = head_forward_bits(CASES[k])
    assert sha == str(z[f"x_sha256_{k}"]), "the input generator changed, not the kernel: regenerate the fixture"
    assert np.array_equal(logits, z[f"logits_{k}"])
    assert np.array_equal(loss, z[f"loss_{k}"])
