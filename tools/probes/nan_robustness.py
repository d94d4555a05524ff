"""Non-finite states must come out as non-finite numbers, not as a crash -- and now as assertions, not as a probe: this file's cases (a NaN in
sample 0 of X_seq through one small csr-fixed train step per kernel family: c32, c64, c32k3, small-graph C = 5) are
``tests/test_nonfinite.py::test_module_hands_a_nan_sample_on_like_the_twin`` (GPU model against the CPU twin's run of the same schedule) and
``test_module_on_the_cpu_twin_flags_the_poisoned_sample``; the per-kernel contract (include/stc_hip.h, "Non-finite values") is the rest of that
file.  Run them with

    python -m pytest tests/test_nonfinite.py -q -m gpu
"""
if __name__ == '__main__':
    print(__doc__)
