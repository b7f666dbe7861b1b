"""Side-buffer sizes of the attention entry points at head_dim 128, with and without
NSTL_ATTN_DH128_OK: pure host arithmetic, no GPU.  Runs in a child process like
tests/test_attn_ragged_sizes.py (the library is never loaded into the CPU suite's own
process).  (mask words, bias rows) are (0, 0) exactly where the call goes generic."""
from tests.test_abi import run_child

SIZES = """
        from neurosync_trainer_lite_amd import _hip as K
        B, H = 2, 3
        R, W = K.ATTN_RAGGED_OK, K.ATTN_DH128_OK
        def sizes(T, flags, dtype=K.BF16, dh=128):
            a = K.attn_args(dtype, B, T, H, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0, 0, dh=dh, flags=flags)
            return K.attn_mask_words(a), K.attn_bias_rows(a)
"""


def test_flag_value_and_version():
    run_child("""
        from neurosync_trainer_lite_amd import _hip as K
        assert K.ATTN_DH128_OK == 2 and K.ATTN_RAGGED_OK == 1
        assert K.lib().nstl_version() >= 3
    """)


def test_without_the_flag_head_dim_128_stays_generic():
    run_child(SIZES + """
        for T in (128, 288, 300):
            assert sizes(T, 0) == (0, 0), T
            assert sizes(T, R) == (0, 0), T
    """)


def test_mask_words_and_bias_rows_with_the_flag():
    run_child(SIZES + """
        # whole tiles: every length streams, T <= 256 included
        assert sizes(128, W) == (B * H * 256, B)
        assert sizes(288, W) == (B * H * 18 * 18 * 4, 3 * B)
        assert sizes(128, W | R) == sizes(128, W)
        assert sizes(32, W) == (B * H * 2 * 2 * 4, B)
        assert sizes(4096, W) == (B * H * 256 * 256 * 4, 32 * B)
        # ragged: both flags
        assert sizes(300, W) == (0, 0)
        assert sizes(300, W | R) == (B * H * 19 * 19 * 4, 3 * B)
        assert sizes(7, W | R) == (B * H * 4, B)
        assert sizes(7, W) == (0, 0)
    """)


def test_f32_and_other_head_widths_stay_generic():
    run_child(SIZES + """
        for T in (128, 288, 300):
            assert sizes(T, W | R, dtype=K.F32) == (0, 0), T
            for dh in (32, 96, 256):
                assert sizes(T, W | R, dh=dh) == (0, 0), (T, dh)
        # head_dim 64 does not read the bit
        for T in (128, 288, 300):
            assert sizes(T, W | R, dh=64) == sizes(T, R, dh=64) != (0, 0), T
            assert sizes(T, W, dh=64) == sizes(T, 0, dh=64), T
    """)


def test_long_env_switch_sends_head_dim_128_generic():
    run_child(SIZES + """
        import os
        assert sizes(128, W | R) != (0, 0) and sizes(300, W | R) != (0, 0)
        os.environ["NSTL_ATTN_LONG"] = "0"
        for T in (7, 128, 288, 300):
            assert sizes(T, W | R) == (0, 0), T
        del os.environ["NSTL_ATTN_LONG"]
        os.environ["NSTL_ATTN_RAGGED"] = "0"    # keeps its meaning: the ragged lengths only
        assert sizes(300, W | R) == (0, 0)
        assert sizes(288, W | R) == (B * H * 18 * 18 * 4, 3 * B)
    """)


def test_attn_set_rejects_a_small_mask():
    run_child("""
        import torch
        from neurosync_trainer_lite_amd import _hip as K
        B, H, T = 2, 3, 300
        a = K.attn_args(K.BF16, B, T, H, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.3, 0, dh=128,
                        flags=K.ATTN_RAGGED_OK | K.ATTN_DH128_OK)
        words = K.attn_mask_words(a)
        assert words == B * H * 19 * 19 * 4
        for n in (B * H * T * T // 64, words - 1):
            try:
                K.attn_set(a, mask_bits=torch.zeros(n, dtype=torch.int64))
            except ValueError:
                pass
            else:
                raise AssertionError("a mask_bits of %d words passed, the call uses %d" % (n, words))
        K.attn_set(a, mask_bits=torch.zeros(words, dtype=torch.int64))
    """)
