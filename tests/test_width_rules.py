"""The host-side width rules that need no device: hidden_dim is a multiple of 128 up
to 2048 (Seq2SeqEngine._check_shapes runs ahead of any device work), and fp8
projections stay with hidden_dim in 256 / 512 / 1024 (the LayerNorm kernels
write the e4m3 side copies at those widths only)."""
import pytest
import torch

from neurosync_trainer_lite_amd.config import training_config
from neurosync_trainer_lite_amd.engine import Seq2SeqEngine
from neurosync_trainer_lite_amd.utils.model_utils import build_model


def model(D, H, **kw):
    cfg = dict(training_config)
    cfg.update(hidden_dim=D, num_heads=H, n_layers=1, dropout=0.0, **kw)
    return build_model(cfg, "cpu")


@pytest.mark.parametrize("D,H", [(192, 3), (2176, 34), (1000, 5)])
def test_unsupported_hidden_dim_is_refused_with_the_rule(D, H):
    m = model(D, H)
    with pytest.raises(ValueError, match=r"multiple of 128 and <= 2048 \(got %d\)" % D):
        Seq2SeqEngine(m, "cpu", torch.float32)


@pytest.mark.parametrize("D,H", [(384, 6), (768, 12), (1152, 18), (2048, 32)])
def test_new_widths_pass_the_shape_check(D, H):
    eng = Seq2SeqEngine.__new__(Seq2SeqEngine)
    eng.D, eng.H, eng.in_dim, eng.out_dim = D, H, 256, 61
    eng._check_shapes()


def test_fp8_at_768_is_refused():
    m = model(768, 12)
    with pytest.raises(ValueError, match=r"fp8 projections need hidden_dim in \(256, 512, 1024\) \(got 768\)"):
        m.set_fp8(True)
    assert not m.fp8
    with pytest.raises(ValueError, match="fp8 projections need hidden_dim"):
        model(768, 12, use_fp8=True)
    # the engine's own entry point, ahead of any launch
    eng = Seq2SeqEngine.__new__(Seq2SeqEngine)
    eng.D, eng.dt = 768, torch.bfloat16
    with pytest.raises(ValueError, match="fp8 projections need hidden_dim"):
        eng.set_fp8(True)


def test_fp8_stays_at_the_four_widths():
    m = model(256, 4)
    m.set_fp8(True)
    assert m.fp8
