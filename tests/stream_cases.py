"""Helpers of tests/test_side_stream_gpu.py: run a call on a caller's stream in a way that turns an ordering mistake
into a wrong number.

The scheme.  An input of the call under test lives in a *staged* tensor: it holds a **poison** (valid input of the same
shape and dtype: the volume reversed, the activation negated, the mask inverted) until a device-to-device copy writes
the **true** input over it -- and that copy is enqueued on the side stream behind a **delay** of tens of milliseconds
of torch work.  The call comes next on the same stream; every device result is cloned right behind it, still on that
stream.  Whatever part of the call runs on another stream (the context's private one, the null stream, a stream
remembered from an earlier call) runs *now*, not behind the delay: it reads the poison, or its result is cloned before
it exists.  Nothing is uninitialised and nothing is out of range, so a mistake is a wrong number, never a fault.

A **poison pass** precedes the real one on the same stream: the call runs once on the poison itself and is
synchronised.  Without it the caching allocator's blocks and the context's scratch would still hold what the warm-up
on the default stream left there -- the very numbers the side-stream run is compared with -- and a result read too
early would look right.  After the poison pass a stale read gives the poison's result.

Nothing here is a pytest file: no fixtures, no settings.  Only public torch operations are used (no kernel of this
project, no spinning on a flag, no graph capture)."""
import math

import numpy as np
import torch

TARGET_MS = 60.0                 # what ``delay`` is sized for
MIN_MS, MAX_MS = 20.0, 500.0     # what the control accepts of the delay it measured
_SCRATCH_ELEMS = 1 << 26         # fp32: 256 MiB read and written per operation of the chain
_state = {}


def side():
    """A fresh side stream (torch's pool streams are non-blocking: nothing orders them against the null stream) on
    which the default stream does not wait.  The runtime multiplexes its streams onto a few hardware queues, and two
    streams that share one run their work in the order it was submitted: on such a stream the default stream's work
    queues up behind the delay and no ordering error can show.  So fresh streams are drawn until a probe finds one the
    default stream runs ahead of (the verdict is kept per stream handle; the pool hands a handle out again later)."""
    verdicts = _state.setdefault("free", {})
    s = None
    for _ in range(64):
        s = torch.cuda.Stream()
        if s.cuda_stream not in verdicts:
            verdicts[s.cuda_stream] = _runs_ahead(torch.cuda.default_stream(), s)
        if verdicts[s.cuda_stream]:
            return s
    return s                                   # none: the control says so


def side_pair():
    """Two side streams as ``side`` gives them that do not wait for one another either.  A launch that lands on some
    third stream (the context's private one, a stream remembered from an earlier call) can share a hardware queue with
    one of the two and so hide behind its delay, but not with both: every case runs on each."""
    a = side()
    b = None
    for _ in range(64):
        b = side()
        if b.cuda_stream != a.cuda_stream and _runs_ahead(b, a):
            return a, b
    return a, b


def _runs_ahead(free, busy):
    """Does work enqueued on ``free`` complete while ``busy`` is still working?  (About 10 ms of chain on ``busy``, then
    one small operation on ``free``.)"""
    _calibrate()
    done_busy, done_free = torch.cuda.Event(), torch.cuda.Event()
    with torch.cuda.stream(busy):
        _chain(_state["buf"], max(1, int(math.ceil(10.0 / _state["per_ms"]))))
        done_busy.record(busy)
    with torch.cuda.stream(free):
        _state["small"].add_(1.0)
        done_free.record(free)
    done_free.synchronize()
    ahead = not done_busy.query()
    done_busy.synchronize()
    return ahead


def _chain(buf, reps):
    for _ in range(reps):
        buf.mul_(0.5).add_(1.0)          # stays finite for any number of repetitions (fixed point 2)


def _calibrate():
    """Once per session: time the chain with two events and size it for TARGET_MS."""
    if "reps" in _state:
        return
    buf = torch.zeros(_SCRATCH_ELEMS, dtype=torch.float32, device="cuda")
    _chain(buf, 8)                                        # clocks up, kernels loaded
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    _chain(buf, 32)
    t1.record()
    t1.synchronize()
    per = max(t0.elapsed_time(t1) / 32.0, 1e-3)
    _state.update(buf=buf, small=torch.zeros(64, device="cuda"), per_ms=per,
                  reps=max(1, int(math.ceil(TARGET_MS / per))))
    torch.cuda.synchronize()


def delay(stream, timed=False):
    """Keep ``stream`` busy for about TARGET_MS with a chain of element-wise torch operations on one scratch tensor.
    ``timed``: returns the (start, end) events around the chain."""
    _calibrate()
    with torch.cuda.stream(stream):
        ev = None
        if timed:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record(stream)
        _chain(_state["buf"], _state["reps"])
        if timed:
            ev[1].record(stream)
    return ev


class Staged:
    """A device tensor (``tensor``) that holds ``poison`` until ``release`` copies ``true`` over it."""

    def __init__(self, true, poison):
        assert true.is_cuda and poison.is_cuda and true.shape == poison.shape and true.dtype == poison.dtype
        self.true = true.detach().clone()
        self.poison = torch.empty_like(self.true)          # the true tensor's layout, whatever op made the poison
        self.poison.copy_(poison.detach())
        self.tensor = self.poison.clone()
        assert self.true.stride() == self.poison.stride() == self.tensor.stride()
        assert not torch.equal(_bits(self.true), _bits(self.poison)), "the poison equals the true input"
        torch.cuda.synchronize()

    def arm(self):
        """``tensor`` <- poison, on the current stream."""
        with torch.no_grad():
            self.tensor.copy_(self.poison)

    def release(self):
        """``tensor`` <- true, a device-to-device copy on the current stream."""
        with torch.no_grad():
            self.tensor.copy_(self.true)

    def fresh(self):
        """A new tensor holding the true input (for the runs on the default stream)."""
        return self.true.clone()


def staged(true, poison):
    return Staged(true, poison)


def reversed_z(t):
    """The poison of a volume of counts or fp32 values: the same values, mirrored along the first axis."""
    return torch.flip(t, dims=[0]).contiguous()


def _bits(t):
    t = t.detach()
    if t.dtype == torch.bool:
        return t
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def clone_tree(out):
    """Every device tensor of a result (nested tuples, lists, dicts) cloned on the current stream."""
    if isinstance(out, torch.Tensor):
        return out.detach().clone() if out.is_cuda else out
    if isinstance(out, (tuple, list)):
        return type(out)(clone_tree(o) for o in out)
    if isinstance(out, dict):
        return {k: clone_tree(v) for k, v in out.items()}
    return out


def run_on_default(fn, *inputs):
    """The baseline and the warm-up: ``fn`` on fresh copies of the true inputs on the default stream."""
    args = [i.fresh() if isinstance(i, Staged) else i for i in inputs]
    out = clone_tree(fn(*args))
    torch.cuda.synchronize()
    return out


def run_on_side(fn, *inputs, stream=None, poison_pass=True):
    """``fn`` on a side stream, behind the delay and the copies that turn the staged inputs from poison into their
    true values; every device result cloned on that stream right after ``fn`` returns.  Inputs that are no ``Staged``
    (tables, patch starts, coded streams) are passed as they are.  Between the producers and the clones there is no
    ``torch.cuda.synchronize()`` and no operation on the default stream."""
    s = stream if stream is not None else side()
    held = [i for i in inputs if isinstance(i, Staged)]
    args = [i.tensor if isinstance(i, Staged) else i for i in inputs]
    for i in held:
        i.arm()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        if poison_pass:
            out = fn(*args)
            del out
            for i in held:                 # fn may write its inputs in place
                i.arm()
            s.synchronize()
        delay(s)
        for i in held:
            i.release()
        out = clone_tree(fn(*args))
    s.synchronize()
    return out


def same(a, b, what=""):
    """Bit-for-bit equality of two results (tensors by their bytes, so NaNs compare too; numpy arrays; numbers)."""
    if isinstance(a, torch.Tensor):
        assert isinstance(b, torch.Tensor) and a.shape == b.shape and a.dtype == b.dtype, what
        differ = int((_bits(a) != _bits(b)).sum())
        assert differ == 0, f"{what}: {differ} of {a.numel()} elements differ from the default-stream result"
    elif isinstance(a, np.ndarray):
        np.testing.assert_array_equal(a.view(np.uint8) if a.dtype.kind == "f" else a,
                                      b.view(np.uint8) if b.dtype.kind == "f" else b, err_msg=what)
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), what
        for k, (x, y) in enumerate(zip(a, b)):
            same(x, y, f"{what}[{k}]")
    elif isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for k in a:
            same(a[k], b[k], f"{what}[{k!r}]")
    elif isinstance(a, float) and math.isnan(a):
        assert isinstance(b, float) and math.isnan(b), what
    else:
        assert a == b, f"{what}: {a!r} != {b!r}"


# ---- the control ----------------------------------------------------------------------------------------------------
def control():
    """Is the delay long enough, and are the streams independent enough, for this harness to see an ordering error on
    the machine at hand?  Torch operations only.  With the delay and the producer on a side stream, a ``clone`` of the
    staged tensor enqueued on the *default* stream must return the poison and one enqueued on the side stream the true
    values.  Returns a dict with ``ok``, ``message`` and the measured ``delay_ms``; computed once per session."""
    if "control" in _state:
        return _state["control"]
    g = torch.Generator(device="cuda").manual_seed(5)
    true = torch.randn(1 << 16, generator=g, device="cuda")
    st = staged(true, -true)
    s = side()
    with torch.cuda.stream(s):
        t0, t1 = delay(s, timed=True)
        st.release()
    early = st.tensor.clone()                          # on the default stream: nothing orders it behind the delay
    with torch.cuda.stream(s):
        late = st.tensor.clone()
    torch.cuda.synchronize()
    ms = float(t0.elapsed_time(t1))
    problems = []
    if not MIN_MS <= ms <= MAX_MS:
        problems.append(f"the delay took {ms:.1f} ms, outside [{MIN_MS:g}, {MAX_MS:g}] ms")
    if not torch.equal(early, st.poison):
        problems.append("a clone enqueued on the default stream did not see the poison: the default stream waited for "
                        "the side stream, an ordering error would be invisible")
    if not torch.equal(late, st.true):
        problems.append("a clone enqueued on the side stream did not see the true values")
    _state["control"] = {"ok": not problems, "message": "; ".join(problems), "delay_ms": ms,
                         "reps": _state["reps"], "per_ms": _state["per_ms"]}
    return _state["control"]


def require_control():
    """First line of every side-stream test: fail (never skip) when the control does not hold."""
    c = control()
    assert c["ok"], "the side-stream control failed, so this test could not see an ordering error: " + c["message"]
