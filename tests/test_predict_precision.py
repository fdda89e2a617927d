"""predict(precision=...) outside the GPU: the argument is checked before any device work, and the element-type
codes of the dtype-coded NDHWC entries agree between include/exabm4d.h and the ctypes binding (CPU)."""
import os
import re

import numpy as np
import pytest

from aind_exaspim_image_compression import _native, inference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("precision", ["fp8", "FP16", "float16", "half", "", None, 16])
def test_unknown_precision_is_a_value_error_before_device_work(precision):
    calls = []

    def model(batch):
        calls.append(batch)
        return batch
    with pytest.raises(ValueError, match="precision"):
        inference.predict(np.zeros((64, 64, 64), np.uint16), model, None, verbose=False, precision=precision)
    assert not calls


def test_precisions():
    assert set(inference.PRECISIONS) == {"fp32", "fp16", "bf16"} and inference.PRECISIONS["fp32"] is None


def test_dtype_codes_match_the_header():
    text = open(os.path.join(ROOT, "include", "exabm4d.h")).read()
    codes = dict((k, int(v)) for k, v in re.findall(r"EXABM4D_DTYPE_(\w+)\s*=\s*(\d+)", text))
    assert codes == {"F32": _native.DTYPE_F32, "F16": _native.DTYPE_F16, "BF16": _native.DTYPE_BF16}
