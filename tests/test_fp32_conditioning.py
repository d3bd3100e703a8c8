"""Problem #50 of the 64-problem C5 case is the fp64 oracle's own worst-conditioned problem,
by a wide margin, in every output array -- shown on the CPU from the oracle alone
(tests/_conditioning.py).  That is why tests/test_gpu_fp32.py allows the fp32 solve its
largest error there and nowhere else.

Measured (sens, eight perturbations of fp32-rounding size): median over problems / second
worst (problem) / #50: X 6.6e-6 / 1.2e-4 (15) / 8.1e-4, U 2.7e-6 / 9.7e-5 (63) / 4.6e-4,
K 2.5e-6 / 5.8e-5 (22) / 6.2e-4, DU 1.8e-6 / 4.3e-5 (63) / 3.7e-4, G 2.8e-6 / 1.1e-4 (63) /
3.4e-3: #50 stands 4.7x to 31x above the second worst and 123x to 1200x above the median."""
import numpy as np
import pytest

import _conditioning as C


def test_problem_50_is_the_oracles_worst_conditioned():
    import oracle as O
    if not O.available():
        pytest.skip("oracle not built")
    _, sens, kept = C.c5_sensitivity()
    assert kept, "a perturbed oracle solve changed a decision trace"
    for k in C.ARRAYS:
        s = sens[k]
        srt = np.sort(s)
        print(f"oracle sensitivity {k}: median {np.median(s):.2e}, second worst {srt[-2]:.2e} "
              f"(problem {np.argsort(s)[-2]}), worst {srt[-1]:.2e} (problem {s.argmax()})")
        assert s.argmax() == C.WORST, (k, s.argmax())
        assert srt[-1] >= 3 * srt[-2], (k, srt[-1] / srt[-2])
        assert srt[-1] >= 50 * np.median(s), (k, srt[-1] / np.median(s))
