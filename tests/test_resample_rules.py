"""The host-side rules of the device resampler, through the C ABI without a device:
nstl_resample_out_len, every rejection of nstl_resample_poly / nstl_peak_normalise (each
names its limit and returns before any device work: the pointers handed over are never
followed) and version 7 of the ABI.  In a child process, as tests/test_abi.py does."""
from tests import resample_ref as R
from tests.test_abi import run_child


def test_out_len_is_ceil_and_zero_for_bad_arguments():
    cases = [(n, up, down) for up, down in R.RATIOS for n in (1, 2, 37, 1000, R.n_in_past_three_runs(up, down))]
    cases += [(1 << 29, 441, 80), (1 << 47, 16384, 1), ((1 << 48) - 1, 16384, 16384)]
    want = [R.out_len(*c) for c in cases]
    run_child("""
        from neurosync_trainer_lite_amd import _hip as K
        cases, want = eval(sys.argv[1]), eval(sys.argv[2])
        assert [K.resample_out_len(*c) for c in cases] == want
        for bad in [(0, 2, 1), (-5, 2, 1), (10, 0, 1), (10, 1, 0), (10, 16385, 1), (10, 1, 16385), (10, -1, 1),
                    (1 << 48, 16384, 1), (1 << 61, 2, 1)]:
            assert K.resample_out_len(*bad) == 0, bad
        assert K.resample_out_len((1 << 61) - 1, 2, 1) == (1 << 62) - 2
    """, repr(cases), repr(want))


def test_rejections_name_their_limit_and_version_7():
    run_child("""
        import ctypes
        from neurosync_trainer_lite_amd import _hip as K
        lib = K.lib()
        assert lib.nstl_version() >= 7
        fields = [f[0] for f in K.ResampleArgs._fields_]
        assert fields == ["x", "n_in", "up", "down", "taps", "n_taps", "y", "n_out", "peak"]

        def call(**change):
            # valid but for `change`; 64 is no device address and is never read
            v = dict(x=64, n_in=1000, up=147, down=80, taps=64, n_taps=2941, y=64, n_out=1838, peak=None)
            v.update(change)
            a = K.ResampleArgs(**v)
            rc = lib.nstl_resample_poly(ctypes.byref(a), None)
            return rc, lib.nstl_last_error_string().decode()

        for change, words in [
                (dict(x=None), ["null pointer"]), (dict(taps=None), ["null pointer"]), (dict(y=None), ["null pointer"]),
                (dict(n_in=0), ["n_in 0 < 1"]), (dict(n_in=-3), ["n_in -3 < 1"]),
                (dict(up=0), ["up 0", "[1, 16384]"]), (dict(up=16385, n_taps=20 * 16385 + 1), ["up 16385", "[1, 16384]"]),
                (dict(down=0), ["down 0", "[1, 16384]"]), (dict(down=16385), ["down 16385", "[1, 16384]"]),
                (dict(n_taps=2940), ["n_taps 2940", "20 max(up, down) + 1 = 2941"]),
                (dict(n_taps=20 * 80 + 1), ["n_taps 1601", "2941"]),
                (dict(n_out=1837), ["n_out 1837", "1838"]), (dict(n_out=1839), ["n_out 1839", "1838"]),
                (dict(n_in=1 << 48, up=16384, down=1, n_taps=20 * 16384 + 1, n_out=1 << 62), [">= 2^62"])]:
            rc, msg = call(**change)
            assert rc == 1, (change, rc, msg)          # hipErrorInvalidValue: the argument check, not a launch
            assert msg.startswith("nstl_resample_poly:") and all(w in msg for w in words), (change, msg)
        assert lib.nstl_resample_poly(None, None) == 1 and "null args" in lib.nstl_last_error_string().decode()

        for args, word in [((None, 10, 64), "null pointer"), ((64, 10, None), "null pointer"), ((64, -1, 64), "n -1 < 0")]:
            assert lib.nstl_peak_normalise(args[0], args[1], args[2], None) == 1
            assert word in lib.nstl_last_error_string().decode()
        assert lib.nstl_peak_normalise(64, 0, 64, None) == 0    # nothing to do, nothing launched
    """)
