"""The write side that the store-to-store operators share (``utils/store_windows.py``), no GPU: the check of ``chunks``,
the clock of the phases, and that ``predict_store`` and ``denoise_store`` refuse a bad ``chunks`` as the others do."""
import numpy as np
import pytest

from aind_exaspim_image_compression import _native, inference
from aind_exaspim_image_compression.bm4d import denoise_store
from aind_exaspim_image_compression.utils import store_windows


def test_check_chunks_takes_five_positive_sizes_after_two_ones():
    assert store_windows.check_chunks(None) is None
    assert store_windows.check_chunks((1, 1, 8, 16, 32)) == (1, 1, 8, 16, 32)
    got = store_windows.check_chunks([np.int64(1), np.int32(1), np.uint16(8), np.int64(16), np.int8(32)])
    assert got == (1, 1, 8, 16, 32) and all(type(c) is int for c in got)


@pytest.mark.parametrize("bad", [5, (1, 1, 8, 8), (1, 2, 8, 8, 8), (1, 1, 0, 8, 8)])
def test_check_chunks_refuses_anything_else(bad):
    with pytest.raises(ValueError, match=r"chunks must be \(1, 1, cz, cy, cx\)"):
        store_windows.check_chunks(bad)


@pytest.mark.parametrize("timed", [True, False])
def test_the_clock_synchronises_once_per_reading_and_only_when_timed(timed):
    syncs = []
    clock = store_windows.PhaseClock(("read", "encode"), timed, lambda: syncs.append(1))
    assert clock.seconds == {"read": 0.0, "encode": 0.0} and syncs == []
    t = [clock() for _ in range(3)]
    assert len(syncs) == (3 if timed else 0)
    assert t[0] <= t[1] <= t[2]
    clock.seconds["read"] += t[2] - t[0]
    assert clock.seconds["read"] >= 0.0 and clock.seconds["encode"] == 0.0


@pytest.fixture
def no_context(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a device context was asked for before the arguments were checked")

    monkeypatch.setattr(_native, "context", refuse)
    monkeypatch.setattr(_native, "Context", refuse)


def test_predict_store_and_denoise_store_refuse_chunks_that_are_no_sequence(tmp_path, no_context):
    src, dst = str(tmp_path / "no-such-store"), str(tmp_path / "dst")
    with pytest.raises(ValueError, match="chunks must be"):
        inference.predict_store(src, dst, model=lambda x: x, transform=None, verbose=False, chunks=5)
    with pytest.raises(ValueError, match="chunks must be"):
        denoise_store(src, dst, 24.0, 37.0, chunk=32, halo=4, chunks=5)
    assert not (tmp_path / "dst").exists()
