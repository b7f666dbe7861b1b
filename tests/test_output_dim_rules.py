"""The host-side rules of output_dim up to 128 that need no device: the engine's shape
check, the model's head, version 6 of the ABI (nstl_loss_args.flags, the loss_wide
counter), and the fused loss's argument check, which runs ahead of any device work."""
import ctypes

import pytest
import torch

from neurosync_trainer_lite_amd import _hip as K
from neurosync_trainer_lite_amd.config import training_config
from neurosync_trainer_lite_amd.engine import Seq2SeqEngine
from neurosync_trainer_lite_amd.utils.model_utils import build_model


def bare_engine(out_dim):
    eng = Seq2SeqEngine.__new__(Seq2SeqEngine)
    eng.D, eng.H, eng.in_dim, eng.out_dim = 256, 4, 256, out_dim
    return eng


@pytest.mark.parametrize("out_dim", [65, 68, 128])
def test_wide_output_dim_passes_the_shape_check(out_dim):
    bare_engine(out_dim)._check_shapes()


def test_output_dim_129_is_refused_with_the_rule():
    with pytest.raises(ValueError, match=r"output_dim must be <= 128 \(got 129\)"):
        bare_engine(129)._check_shapes()


def test_build_model_with_68_outputs():
    cfg = dict(training_config)
    cfg.update(hidden_dim=128, num_heads=2, n_layers=1, dropout=0.0, output_dim=68)
    m = build_model(cfg, "cpu")
    assert tuple(m.decoder.fc_output.weight.shape) == (68, 128)
    assert tuple(m.decoder.fc_output.bias.shape) == (68,)


def test_abi_version_6():
    assert K.lib().nstl_version() >= 6


def test_loss_args_end_with_the_flags_field():
    fields = [f[0] for f in K.LossArgs._fields_]
    assert fields[-2:] == ["loss_out", "flags"]
    assert K.LossArgs.flags.size == 4 and K.LossArgs.flags.offset == K.LossArgs.loss_out.offset + 8
    assert ctypes.sizeof(K.LossArgs) >= K.LossArgs.loss_out.offset + 8 + 4
    assert K.LossArgs().flags == 0, "a caller that never sets flags must get the behaviour of version 5"
    assert K.LOSS_WIDE_OK == 1


def test_loss_wide_counter_exists_and_resets():
    assert K.KERNEL_COUNT_NAMES[-1] == "loss_wide" and K.KERNEL_COUNT_NAMES[-2] == "attn_bwd_long"
    K.kernel_counts_reset()
    counts = K.kernel_counts()  # raises if the library's counter count differs from the bindings'
    assert counts["loss_wide"] == 0


def loss_args(F, flags, T=4, ld=136):
    """A call that would be valid but for its shape; the pointers are never followed by
    the argument check (and no check that fails leaves one to follow)."""
    a = K.LossArgs()
    a.B, a.T, a.F = 1, T, F
    a.pred, a.pred_ld, a.trg, a.trg_ld = 4096, ld, 4096, ld
    a.delta, a.w1, a.w2, a.w3, a.grad_scale = 1.0, 1.0, 1.0, 1.0, 1.0
    a.dpred, a.dpred_dtype, a.dpred_ld = 4096, K.F32, ld
    a.partial, a.loss_out = 4096, 4096
    a.flags = flags
    return a


@pytest.mark.parametrize("F,flags,limit", [(65, 0, "F <= 64"), (129, K.LOSS_WIDE_OK, "F <= 128"),
                                           (129, 0, "F <= 64"), (0, K.LOSS_WIDE_OK, "F <= 128")])
def test_loss_shape_rejections_name_the_limit(F, flags, limit):
    lib = K.lib()
    K.kernel_counts_reset()
    rc = lib.nstl_loss_fwd_bwd(ctypes.byref(loss_args(F, flags)), None)
    msg = lib.nstl_last_error_string().decode()
    assert rc == 1, rc  # hipErrorInvalidValue: an argument error
    assert "unsupported" in msg and limit in msg and "F=%d" % F in msg, msg
    assert not any(K.kernel_counts().values()), "a rejected call launched"


@pytest.mark.parametrize("kw,text", [(dict(T=4097), "T in [2,4096]"), (dict(T=1), "T in [2,4096]"), (dict(ld=64), "ld < F")])
def test_loss_wide_rejections_whatever_the_flags(kw, text):
    lib = K.lib()
    for flags in (0, K.LOSS_WIDE_OK):
        F = 68 if flags else 61
        if "ld" in kw:
            kw = dict(ld=56)
        rc = lib.nstl_loss_fwd_bwd(ctypes.byref(loss_args(F, flags, **kw)), None)
        msg = lib.nstl_last_error_string().decode()
        assert rc == 1 and text in msg, (flags, rc, msg)
