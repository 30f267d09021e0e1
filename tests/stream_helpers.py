"""The probe of tests/test_gpu_caller_stream.py: a caller's stream that is provably still busy while a wrapper is called under it.

``held_stream()`` yields a fresh non-blocking stream S with a bounded delay queued on it (``torch.cuda._sleep``: a clock spin of a
fixed number of cycles, not a wait on a flag) and an event ``started`` recorded right behind the delay.  While ``started`` has not
completed, nothing queued on S behind it has run: work a wrapper launches on another stream runs at once and reads inputs that are
still NaN, and a clone queued on S behind a wrapper that forgot a join runs before the work it should have waited for.

``probe()`` runs one case the way DESIGN.md §6.7b describes it.  The conditions that keep a case from passing
vacuously are asserted, never skipped:

* ``started.query()`` is False immediately before the wrapper is called and, for wrappers that do not block the host, immediately
  after it returns (``HOST_BLOCKING`` names the wrappers that block by design: they are checked before the call only);
* the legacy null stream really runs past S.  The runtime multiplexes its streams onto a few hardware queues, and two streams that
  share a queue run in order whatever the program says; a stream on which that happens is let go and another one is taken.
"""
import contextlib

import torch

TARGET_MS = 50.0         # about ten times the host enqueue of a whole training step (163 dispatches, a few milliseconds)
CAP_MS = 200.0           # no single delay may be longer
CALIBRATION_CYCLES = 2_000_000
TRIES = 12               # sets of fresh streams tried until one shares no hardware queue with the streams that must run past it

# Wrappers that block the host inside the call, by design: ``started`` is checked before the call only (behind the block the delay
# has run out).  Name of the case's wrapper -> what blocks.
HOST_BLOCKING = {
    "forward_prepared(lengths)": "ops.device_lengths uploads the lengths from pageable host memory",
    "stoi": "metrics.stoi_clips uploads its clip table from pageable host memory",
    "loudness": "LoudnessMeter.clips uploads its clip table from pageable host memory",
    "embed_many": "SpeakerEncoder.embed_many uploads the frame and window offsets from pageable host memory",
    "shoebox_rir": "reverb.shoebox_rir uploads the room descriptors from pageable host memory",
    "RirPool": "shoebox_rir, and the tap counts go up from pageable host memory",
    "bilstm_recurrent_train": "_lstm_check_err reads the error word of the persistent recurrence back",
    "lstm_status": "reads the error word of the last training step back",
}

_state = {}


def delay_cycles() -> int:
    """Cycles of one delay: one ``_sleep`` of a fixed count is timed between two events (behind a first one that loads the kernel)
    and scaled to TARGET_MS.  Done once per process."""
    if "cycles" not in _state:
        s = torch.cuda.Stream()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            torch.cuda._sleep(CALIBRATION_CYCLES)
            t0.record()
            torch.cuda._sleep(CALIBRATION_CYCLES)
            t1.record()
        s.synchronize()
        ms = t0.elapsed_time(t1)
        assert ms > 0.0, "torch.cuda._sleep took no time: the delay cannot be calibrated"
        _state["cycles"] = max(1, int(CALIBRATION_CYCLES * TARGET_MS / ms))
        print(f"stream probe: {CALIBRATION_CYCLES} sleep cycles took {ms:.3f} ms; one delay = {_state['cycles']} cycles (target {TARGET_MS:.0f} ms)")
    return _state["cycles"]


def _tick(stream) -> None:
    """A tiny kernel on ``stream`` and a host wait for it (for that kernel alone, not for the device)."""
    if "tick" not in _state:
        _state["tick"] = torch.zeros(64, device="cuda")
        torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        _state["tick"].add_(1.0)
    ev = torch.cuda.Event()
    ev.record(stream)
    ev.synchronize()


class Held:
    """A stream with a delay in flight.  ``before()`` / ``after()`` are the conditions around a wrapper call."""

    def __init__(self, label: str, poison=()):
        self.label = label
        self.stream = torch.cuda.Stream()
        if poison:
            poison_pool(self.stream, poison)
        self._t0 = torch.cuda.Event(enable_timing=True)
        self.started = torch.cuda.Event(enable_timing=True)
        self.checks = []
        self.delay_ms = None
        self.free = []
        with torch.cuda.stream(self.stream):
            self._t0.record()
            torch.cuda._sleep(delay_cycles())
            self.started.record()

    def _check(self, when: str):
        done = self.started.query()
        self.checks.append(f"{when}: started={done}")
        assert not done, (f"{self.label}: the delay on the caller's stream had run out {when} -- the case would prove nothing "
                          f"(checks so far: {self.checks})")

    def before(self):
        self._check("before the call")

    def after(self, wrapper: str = None):
        if wrapper in HOST_BLOCKING:
            self.checks.append(f"after the call: not checked ({wrapper} blocks the host: {HOST_BLOCKING[wrapper]})")
            return
        self._check("after the call")

    def close(self):
        self.stream.synchronize()
        self.delay_ms = self._t0.elapsed_time(self.started)
        print(f"{self.label}: delay {self.delay_ms:.1f} ms; " + "; ".join(self.checks))
        return self.delay_ms


def _hold(labels, poison=(), free=0):
    """One ``Held`` per label, none of whose delays has run out yet, which the legacy null stream runs past -- and ``free`` more
    fresh streams that run past them too (the second stream of a build-on-one, use-on-another case).  A stream that shares a
    hardware queue with a held one waits behind its delay and so uses it up: then the whole set is let go and made again."""
    null = torch.cuda.default_stream()
    for attempt in range(TRIES):
        group = [Held(label, poison) for label in labels]
        others = []
        while len(others) < free:
            s = torch.cuda.Stream()
            if all(s != h.stream for h in group) and s not in others:
                others.append(s)
        for s in [null] + others:
            _tick(s)
        if not any(h.started.query() for h in group):
            for h in group:
                h.checks.append(f"set {attempt + 1} of streams")
            return group, others
        for h in group:
            h.stream.synchronize()
    raise AssertionError(f"{labels}: no set of streams out of {TRIES} ran beside one another -- the probe cannot hold one")


@contextlib.contextmanager
def held_streams(labels, poison=(), free=0):
    """``Held`` streams, one per label, queued together; each carries the ``free`` streams of ``_hold`` as ``.free``.  On leaving,
    every held stream is synchronised -- the streams, never the device --, the delays' lengths and the checks are printed, and the
    cap is asserted.  poison: see ``poison_pool``."""
    group, others = _hold(list(labels), poison, free)
    for h in group:
        h.free = others
    try:
        yield group
    except BaseException:
        for h in group:
            h.stream.synchronize()
        raise
    for h in group:
        ms = h.close()
        assert ms <= CAP_MS, f"{h.label}: the delay took {ms:.1f} ms, more than the cap of {CAP_MS:.0f} ms"


@contextlib.contextmanager
def held_stream(label: str = "held stream", poison=(), free=0):
    with held_streams([label], poison, free) as group:
        yield group[0]


def poison_pool(stream, sizes) -> None:
    """Best effort against a stale buffer that happens to hold the right bytes: blocks of ``sizes`` bytes, filled with 0xFF (a NaN
    in every floating-point format), are allocated under ``stream`` and freed again, so that the next ``torch.empty`` of such a
    size under that stream is likely to be handed one of them.  Synchronises the stream, so it runs before the delay is queued."""
    with torch.cuda.stream(stream):
        blocks = [torch.full((int(n),), 0xFF, dtype=torch.uint8, device="cuda") for n in sizes]
    stream.synchronize()
    del blocks


# ---- results ------------------------------------------------------------------------------------------------------------------------
def flatten(out, prefix="out"):
    """A wrapper's result -> [(name, tensor)]: tensors, None, and (nested) tuples, lists and dicts of them."""
    if out is None:
        return []
    if isinstance(out, torch.Tensor):
        return [(prefix, out)]
    if isinstance(out, dict):
        return [p for k in out for p in flatten(out[k], f"{prefix}.{k}")]
    if isinstance(out, (tuple, list)):
        return [p for i, v in enumerate(out) for p in flatten(v, f"{prefix}[{i}]")]
    raise TypeError(f"{prefix}: {type(out).__name__} is not a tensor or a container of tensors")


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    a, b = a.detach().contiguous().reshape(-1), b.detach().contiguous().reshape(-1)
    return torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def keep(out):
    """Clones of a result's tensors, on the current stream, with no synchronisation."""
    return [(n, t.detach().clone()) for n, t in flatten(out)]


def assert_same(label, got, want, finite=True):
    assert [n for n, _ in got] == [n for n, _ in want], (label, [n for n, _ in got], [n for n, _ in want])
    for n, w in want:
        if finite and w.is_floating_point():
            assert torch.isfinite(w).all(), f"{label}: the null-stream {n} is not finite: a NaN read could hide in it"
    bad = [n for (n, g), (_, w) in zip(got, want) if not same_bits(g, w)]
    assert not bad, f"{label}: differs from the null-stream result in {bad}"


def probe(label, call, floats, ints=(), wrapper=None, finite=True):
    """One case.  ``call()`` runs the wrapper on tensors it closes over; ``floats`` are ALL the floating-point device buffers it
    reads (inputs, weights, state it updates in place), ``ints`` the integer buffers it changes in place (restored, never
    poisoned; integer inputs it only reads need no mention: they are written before the delay and left alone).

    1. null stream: the expected result -- twice, from the same start, and both must agree, so that a result that is not
       repeatable is not mistaken for a stream bug; synchronise;
    2. every buffer of ``floats`` is filled with NaN, every buffer of ``ints`` gets its start value back; synchronise;
    3. a held stream S; on S, behind the delay: the real values are copied back into ``floats``; ``started`` must be pending; the
       wrapper is called under S; ``started`` must still be pending (unless ``wrapper`` is in HOST_BLOCKING); the results are
       cloned on S; S -- not the device -- is synchronised;
    4. every result must have the bits of the null-stream run."""
    floats, ints = list(floats), list(ints)
    for t in floats:
        assert t.is_cuda and t.is_floating_point(), f"{label}: floats holds a {t.dtype} tensor on {t.device}"
    with torch.no_grad():
        stage_f = [t.detach().clone() for t in floats]
        stage_i = [t.detach().clone() for t in ints]
    torch.cuda.synchronize()

    def restore():
        with torch.no_grad():
            for t, s in zip(floats + ints, stage_f + stage_i):
                t.detach().copy_(s)

    want = keep(call())
    torch.cuda.synchronize()
    restore()
    again = keep(call())
    torch.cuda.synchronize()
    assert_same(label + " (null stream, rerun)", again, want, finite)
    with torch.no_grad():
        for t, s in zip(ints, stage_i):
            t.detach().copy_(s)
        for t in floats:
            t.detach().fill_(float("nan"))
    torch.cuda.synchronize()
    with held_stream(label) as held:
        with torch.cuda.stream(held.stream):
            with torch.no_grad():
                for t, s in zip(floats, stage_f):
                    t.detach().copy_(s)
            held.before()
            out = call()
            held.after(wrapper)
            got = keep(out)
        held.stream.synchronize()
    assert_same(label, got, want, finite)
    return want
