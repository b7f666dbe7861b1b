"""Side-buffer sizes of the attention entry points at the head widths other than 64 and
128 (any multiple of 8 below 128), with and without NSTL_ATTN_DHANY_OK: pure host
arithmetic, no GPU.  Runs in a child process like tests/test_attn_dh128_sizes.py (the
library is never loaded into the CPU suite's own process).  With the bit a call gets
what a head_dim 128 call of the same B, H, T gets under NSTL_ATTN_DH128_OK; (mask words,
bias rows) are (0, 0) exactly where the call goes generic."""
from tests.test_abi import run_child

SIZES = """
        from neurosync_trainer_lite_amd import _hip as K
        B, H = 2, 3
        R, W, A = K.ATTN_RAGGED_OK, K.ATTN_DH128_OK, K.ATTN_DHANY_OK
        WIDTHS = (8, 24, 32, 56, 72, 96, 120)
        def sizes(T, flags, dtype=K.BF16, dh=32):
            a = K.attn_args(dtype, B, T, H, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0, 0, dh=dh, flags=flags)
            return K.attn_mask_words(a), K.attn_bias_rows(a)
"""


def test_flag_value_and_version():
    run_child("""
        from neurosync_trainer_lite_amd import _hip as K
        assert K.ATTN_DHANY_OK == 4 and K.ATTN_DH128_OK == 2 and K.ATTN_RAGGED_OK == 1
        assert K.lib().nstl_version() >= 4
    """)


def test_sizes_with_the_bit_are_those_of_head_dim_128():
    run_child(SIZES + """
        for dh in WIDTHS:
            for T in (32, 128, 288, 4096):       # whole tiles: the bit alone
                want = sizes(T, W, dh=128)
                assert want != (0, 0), T
                assert sizes(T, A, dh=dh) == want, (dh, T)
                assert sizes(T, A | R, dh=dh) == want, (dh, T)
            for T in (7, 300):                    # ragged: the bit and RAGGED_OK
                want = sizes(T, W | R, dh=128)
                assert want != (0, 0), T
                assert sizes(T, A | R, dh=dh) == want, (dh, T)
        assert sizes(32, A, dh=8) == (B * H * 2 * 2 * 4, B)
        assert sizes(300, A | R, dh=120) == (B * H * 19 * 19 * 4, 3 * B)
    """)


def test_generic_without_the_bit_ragged_without_its_flag_f32_and_other_widths():
    run_child(SIZES + """
        for dh in WIDTHS:
            for T in (7, 32, 128, 288, 300, 4096):
                assert sizes(T, 0, dh=dh) == (0, 0), (dh, T)              # without the bit
                assert sizes(T, R | W, dh=dh) == (0, 0), (dh, T)
                assert sizes(T, A | R | W, dtype=K.F32, dh=dh) == (0, 0), (dh, T)   # f32
            for T in (7, 300):
                assert sizes(T, A, dh=dh) == (0, 0), (dh, T)              # ragged T without RAGGED_OK
                assert sizes(T, A | W, dh=dh) == (0, 0), (dh, T)
        for dh in (4, 12, 136, 256):                                      # not a multiple of 8, or above 128
            for T in (7, 32, 128, 288, 300, 4096):
                assert sizes(T, A | R | W, dh=dh) == (0, 0), (dh, T)
    """)


def test_env_switches_send_the_new_widths_generic():
    run_child(SIZES + """
        import os
        for dh in WIDTHS:
            assert sizes(128, A | R, dh=dh) != (0, 0) and sizes(300, A | R, dh=dh) != (0, 0)
        os.environ["NSTL_ATTN_LONG"] = "0"
        for dh in WIDTHS:
            for T in (7, 32, 128, 288, 300, 4096):
                assert sizes(T, A | R, dh=dh) == (0, 0), (dh, T)
        del os.environ["NSTL_ATTN_LONG"]
        os.environ["NSTL_ATTN_RAGGED"] = "0"    # keeps its meaning: the ragged lengths only
        for dh in WIDTHS:
            for T in (7, 300):
                assert sizes(T, A | R, dh=dh) == (0, 0), (dh, T)
            assert sizes(288, A | R, dh=dh) == (B * H * 18 * 18 * 4, 3 * B), dh
    """)


def test_the_bit_changes_nothing_at_head_dim_64_and_128():
    run_child(SIZES + """
        for T in (7, 32, 128, 288, 300, 4096):
            for base in (0, R, W, R | W):
                for dh in (64, 128):
                    assert sizes(T, base | A, dh=dh) == sizes(T, base, dh=dh), (dh, T, base)
        assert sizes(288, A, dh=128) == (0, 0)              # 128 keeps its own bit
        assert sizes(288, A, dh=64) == sizes(288, 0, dh=64) != (0, 0)
    """)


def test_attn_set_rejects_a_mask_one_word_short():
    run_child("""
        import torch
        from neurosync_trainer_lite_amd import _hip as K
        B, H, T = 2, 3, 300
        for dh in (24, 96):
            a = K.attn_args(K.BF16, B, T, H, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.3, 0, dh=dh,
                            flags=K.ATTN_RAGGED_OK | K.ATTN_DHANY_OK)
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
