"""Streams for the GPU tests that need a kernel to run BESIDE the one under test.  Not a test."""
import torch


def concurrent_side_stream(D, tries=8):
    """A stream whose kernels run beside those of the current stream.

    The runtime serves its streams through a few hardware queues (four by default), so every fourth new stream shares the current
    stream's queue: a long kernel launched there does not compete with the kernel under test for CUs, the kernel under test simply
    queues behind it (measured with 96 CU-squatting workgroups for 400 ms: the whole-chip solve then returns after 371 ms having
    run in one launch, not after 22 ms through the launches).

    No clock decides: one squatter workgroup (dpcg_debug_occupy, 20 ms) goes to the candidate with an event behind it, a tiny kernel
    to the current stream with an event behind it.  Side by side the tiny kernel's event completes while the squatter's is still
    pending; on a shared queue it cannot complete before the squatter's has.  (A host that stalls for the whole 20 ms between the
    two queries can only make a good candidate look shared -- the next one is tried --, never a shared one look good.)"""
    y = torch.zeros(16, device="cuda")
    y.add_(1.0)                                                          # (the tiny kernel, loaded)
    keep = []
    for _ in range(tries):                                               # (of eight consecutive streams at most two share the queue)
        side = torch.cuda.Stream()
        keep.append(side)
        torch.cuda.synchronize()
        D._lib.check(D._lib.lib().dpcg_debug_occupy(1, 20.0, side.cuda_stream))
        squatter_done = torch.cuda.Event()
        squatter_done.record(side)
        y.add_(1.0)
        tiny_done = torch.cuda.Event()
        tiny_done.record(torch.cuda.current_stream())
        tiny_done.synchronize()
        beside = not squatter_done.query()
        side.synchronize()
        if beside:
            return side
    raise AssertionError("no stream runs beside the current one")
