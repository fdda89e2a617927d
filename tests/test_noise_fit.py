"""The Poisson-Gaussian fit of utils/noise.py against numpy's own weighted least squares, and what the module takes
for a device pointer (CPU only).  tests/noise_pyref.py restates the fit with the same steps as the module, so their
equality says nothing about the steps; np.polyfit solves the same problem another way (a scaled SVD least-squares
solve instead of centred sums)."""
import math

import numpy as np
import pytest

import noise_pyref as P

from aind_exaspim_image_compression import _native
from aind_exaspim_image_compression.utils import noise as N

# Two float64 solutions of one well-posed 2-parameter problem differ by about eps * condition.  polyfit scales the
# columns of its design matrix to unit norm, which leaves a condition number below 100 for the curves here (means
# spread over more than a decade); 2.2e-16 * 100, times 50 for the sums of up to 49 terms on either side.
RTOL = 1e-12


def curves():
    rng = np.random.default_rng(11)
    mean = 40.0 * 2.0 ** (np.arange(28) / 4.0)                     # quarter-octave levels, 40 .. 4300 counts
    var = 2.0 * (mean - 100.0) + 64.0 + 100.0 * 2.0                 # gain 2, read noise 8, offset 100 ...
    var = var * (1.0 + 0.03 * rng.standard_normal(mean.size))       # ... scattered, so that the weights matter
    cells = rng.integers(600, 200000, mean.size)
    yield mean, np.sqrt(var), cells, 100.0
    yield mean[:3], np.sqrt(var[:3]), cells[:3], 0.0                # the smallest curve the fit accepts
    yield mean[::-1] * 7.0, np.sqrt(0.5 * mean[::-1] * 7.0 + 9.0), cells, 37.0      # exactly on a line


@pytest.mark.parametrize("fit", [N.fit_poisson_gaussian, P.fit_poisson_gaussian], ids=["module", "pyref"])
def test_fit_equals_numpy_weighted_least_squares(fit):
    for mean, sigma, cells, offset in curves():
        y = sigma ** 2
        # polyfit minimises sum (w_i r_i)^2: its w is the square root of the weight cells / sigma^4
        a, c = np.polyfit(mean, y, 1, w=np.sqrt(cells) / y)
        got = fit(mean, sigma, cells, offset)
        assert got["gain"] == pytest.approx(a, rel=RTOL)
        rn2 = c + a * offset                                        # a sum that may cancel: it loses that much
        assert rn2 > 0.0
        assert got["read_noise"] ** 2 == pytest.approx(rn2, rel=RTOL * (abs(c) + abs(a * offset)) / rn2)
        assert got["offset"] == offset
    exact = fit(*list(curves())[2][:3], 37.0)
    assert exact["gain"] == pytest.approx(0.5, rel=RTOL)
    assert exact["read_noise"] == pytest.approx(math.sqrt(9.0 + 0.5 * 37.0), rel=RTOL)


def test_fit_leaves_out_levels_without_noise():
    mean, sigma, cells, offset = next(curves())
    sigma = sigma.copy()
    sigma[5] = 0.0
    keep = np.arange(mean.size) != 5
    want = N.fit_poisson_gaussian(mean[keep], sigma[keep], cells[keep], offset)
    assert N.fit_poisson_gaussian(mean, sigma, cells, offset) == want


def test_only_gpu_memory_counts_as_resident():
    """A tensor in host memory has a data_ptr too; it must travel as a host array, never as a device address."""
    torch = pytest.importorskip("torch")
    host = torch.zeros(8, dtype=torch.float32)
    assert not N._is_device(host)
    assert not N._is_device(np.zeros(8, np.float32))
    assert N._is_device(1 << 40)

    class OnGpu:
        is_cuda = True

        def data_ptr(self):
            return 1 << 40

    assert N._is_device(OnGpu())
    assert N._is_device(_native.DeviceBuffer.__new__(_native.DeviceBuffer))
