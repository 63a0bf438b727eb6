"""GPU tests (-m gpu) of the launch contract at the top of include/cusp_mi355x.h -- "launches are asynchronous on the given stream",
"no allocation, no synchronisation" -- on every entry point that takes a stream: one case per family and value type of the table in
tests/stream_contract.py (tests/test_stream_contract_inventory.py keeps that table complete).

Check A, classes ASYNC and SYNC: the work is ordered on the stream it is given.  The tensors handed to the entry point hold an
all-zero placeholder (zero row offsets are an empty matrix, index 0 is in range of every dimension >= 1: a launcher that reads them
computes a wrong answer, never an address out of range; structure a PLAN was made from stays in place, plan and arrays must agree);
the outputs hold a sentinel.  On the one side stream of this module -- a torch pool stream: non-blocking, the null stream does not
wait for it -- filler work is queued, behind it the copies of the real inputs into place, and while the filler still runs
(side.query() is False, else the case FAILS as inconclusive) the entry point is called with stream=side.  A SYNC call is compared
as soon as it returns, an ASYNC call after side.synchronize(), both against the reference of the real inputs.  A launch that goes
to the null stream or a private one reads the placeholder; a set-up call that synchronises another stream returns a stale host
value; a later launch of a multi-launch call on another stream than the first runs ahead of its inputs.

Check B, class ASYNC: the call records into a capture.  After one eager warm-up call (module loading and the tuning table stay
outside the capture; its result is compared too) the outputs and the host mirror are refilled with the sentinel and the call is
captured with torch.cuda.graph(g, stream=side) -- global capture mode: an allocation, a synchronisation or a null-stream launch
inside comes back as an error status.  After the capture everything still holds the sentinel (nothing ran eagerly or on a stream
outside the capture); a replay gives the reference; the inputs, device scalars included, are overwritten in place with a second
value set and a second replay gives ITS reference (nothing was read on the host and baked into the launch).  One capture and two
replays per case, one stream, a linear graph.

The filler: FILLER_REPEATS = 64 in-place adds on FILLER_ELEMENTS = 2^28 floats (1 GiB).  Observed on the MI355X: they run 23.0 ms
(five runs, 22.98 .. 23.02) and are queued in 0.4 ms; the first use of the side stream in a process was seen to take 6 ms of host
time once (`test_the_filler_outlasts_the_queueing` runs first and absorbs it).  The copies and the call behind the filler are queued
within a fraction of a millisecond, so the filler outlasts the queueing some fifty times over, and no case of the table came out
inconclusive."""
import pytest

import stream_contract as SC

pytestmark = pytest.mark.gpu

FILLER_ELEMENTS = 1 << 28
FILLER_REPEATS = 64


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def ctx(cmi, orc, torch_cuda):
    return SC.Ctx(cmi, orc, torch_cuda)


@pytest.fixture(scope="module")
def side(torch_cuda):
    return torch_cuda.cuda.Stream()


@pytest.fixture(scope="module")
def filler(torch_cuda):
    buf = torch_cuda.zeros(FILLER_ELEMENTS, dtype=torch_cuda.float32, device="cuda")

    def run():
        for _ in range(FILLER_REPEATS):
            buf.add_(1.0)
    return run


@pytest.fixture(autouse=True)
def stop_after_a_device_fault(torch_cuda):
    """A fault on the device is sticky: nothing after it proves anything, so the session ends there."""
    yield
    try:
        torch_cuda.cuda.synchronize()
    except Exception as e:
        pytest.exit(f"the device reported a fault, stopping: {e}", returncode=3)


def ident(case):
    family, suffix = case
    return f"{family[4:]}-{suffix or 'untyped'}"


def check_a(c, cls, torch, side, filler, what):
    spares = c.spares(0)
    c.placeholders()
    c.reset_outputs()
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(side):
            filler()
            c.queue_inputs(spares)
        assert not side.query(), f"{what}: inconclusive -- the filler had finished before the call was made"
        ret = c.call(side)
        if cls == SC.ASYNC:
            side.synchronize()
        c.check(0, ret)
    finally:
        side.synchronize()


def check_b(c, torch, side, what):
    c.load(0)
    c.reset_outputs()
    torch.cuda.synchronize()
    ret = c.call(side)                      # the eager warm-up
    side.synchronize()
    c.check(0, ret)
    c.load(0)
    c.reset_outputs()
    torch.cuda.synchronize()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    failed = None
    try:
        with torch.cuda.graph(g, stream=side):
            try:
                ret = c.call(side)
            except Exception as e:          # the status of the call says more than what ending a broken capture says
                failed = e
    except Exception as e:
        failed = failed or e
    assert failed is None, f"{what}: the call does not record into a capture: {failed}"
    torch.cuda.synchronize()
    c.assert_untouched(0, f"{what}: during the capture")
    g.replay()
    torch.cuda.synchronize()
    c.check(0, ret)
    c.load(1)
    c.reset_outputs()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    c.check(1, ret)


def test_the_filler_outlasts_the_queueing(torch_cuda, side, filler):
    """Once queued, the filler is still running: what check A's every case rests on."""
    torch = torch_cuda
    filler()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        filler()
    still_running = not side.query()
    side.synchronize()
    assert still_running, "the filler finished while it was being queued: check A would be inconclusive"


@pytest.mark.parametrize("case", SC.cases(SC.ASYNC) + SC.cases(SC.SYNC), ids=ident)
def test_work_is_ordered_on_the_given_stream(ctx, torch_cuda, side, filler, case):
    """Check A."""
    cls = SC.BY_FAMILY[case[0]].cls
    for c in SC.build(ctx, *case):
        try:
            check_a(c, cls, torch_cuda, side, filler, f"{ident(case)} {c.label}".strip())
        finally:
            c.close()


@pytest.mark.parametrize("case", SC.cases(SC.ASYNC), ids=ident)
def test_call_records_into_a_capture(ctx, torch_cuda, side, case):
    """Check B."""
    for c in SC.build(ctx, *case):
        try:
            check_b(c, torch_cuda, side, f"{ident(case)} {c.label}".strip())
        finally:
            c.close()
