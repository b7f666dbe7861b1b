"""Side-buffer sizes of the attention entry points, with and without
NSTL_ATTN_RAGGED_OK: pure host arithmetic, no GPU.  Runs in a child process like
tests/test_abi.py (the library is never loaded into the CPU suite's own process)."""
from tests.test_abi import run_child


def test_mask_words_and_bias_rows():
    run_child("""
        from neurosync_trainer_lite_amd import _hip as K
        B, H = 2, 3
        def sizes(T, flags, dtype=K.BF16, dh=64):
            a = K.attn_args(dtype, B, T, H, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0, 0, dh=dh, flags=flags)
            return K.attn_mask_words(a), K.attn_bias_rows(a)
        F = K.ATTN_RAGGED_OK
        # ragged: the generic kernels without the flag, the streaming ones with it
        assert sizes(300, 0) == (0, 0)
        assert sizes(300, F) == (B * H * 19 * 19 * 4, B * 3)
        assert sizes(257, 0) == (0, 0)
        assert sizes(257, F) == (B * H * 17 * 17 * 4, B * 3)
        assert sizes(7, F) == (B * H * 4, B)
        assert sizes(4095, F) == (B * H * 256 * 256 * 4, B * 32)
        # whole tiles: the flag changes nothing (one-shot kernels at 128)
        assert sizes(128, 0) == sizes(128, F) == (B * H * 128 * 128 // 64, B)
        assert sizes(288, 0) == sizes(288, F) == (B * H * 288 * 288 // 64, B * 3)
        # no streaming kernels for f32 or head_dim 128
        assert sizes(300, F, dtype=K.F32) == (0, 0)
        assert sizes(300, F, dh=128) == (0, 0)
        assert K.lib().nstl_version() >= 2
    """)


def test_ragged_env_switch_sizes():
    run_child("""
        import os
        from neurosync_trainer_lite_amd import _hip as K
        a = K.attn_args(K.BF16, 2, 300, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0, 0, flags=K.ATTN_RAGGED_OK)
        assert K.attn_mask_words(a) > 0
        os.environ["NSTL_ATTN_RAGGED"] = "0"
        assert (K.attn_mask_words(a), K.attn_bias_rows(a)) == (0, 0)
        del os.environ["NSTL_ATTN_RAGGED"]
        os.environ["NSTL_ATTN_LONG"] = "0"
        assert (K.attn_mask_words(a), K.attn_bias_rows(a)) == (0, 0)
    """)


def test_attn_set_rejects_mask_sized_by_the_old_rule():
    run_child("""
        import torch
        from neurosync_trainer_lite_amd import _hip as K
        B, H, T = 2, 3, 300
        a = K.attn_args(K.BF16, B, T, H, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.3, 0, flags=K.ATTN_RAGGED_OK)
        small = torch.zeros(B * H * T * T // 64, dtype=torch.int64)
        try:
            K.attn_set(a, mask_bits=small)
        except ValueError:
            pass
        else:
            raise AssertionError("a T*T/64 mask_bits passed at T = 300 with the flag")
        K.attn_set(a, mask_bits=torch.zeros(K.attn_mask_words(a), dtype=torch.int64))
    """)
