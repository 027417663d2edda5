"""torch hands streams out of a pool of 32 per device, round robin, so the 33rd torch.cuda.Stream of a process is the first again.  The
pipeline's BrushNet side stream is a pool stream, and so is the stream torch.cuda.graph captures on: in a process that has made enough
streams the side stream can BE the stream it forks from, which puts BrushNet and the UNet on one stream and leaves an exported step
program without its fork.  Here the collision is arranged on purpose and _overlap must pick another side stream."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_pipeline_gpu import _tiny_pipe  # noqa: E402


def _second_handle_of(stream):
    for _ in range(64):                                                   # two rounds of the pool
        s = torch.cuda.Stream(device=stream.device)
        if s.cuda_stream == stream.cuda_stream:
            return s
    pytest.fail("no second handle of a pool stream within 64 streams: the pool is not what this test assumes")


@pytest.mark.parametrize("which", ["_side_stream", "_aux_stream"])
def test_the_side_streams_are_never_the_stream_they_fork_from(which):
    pipe = _tiny_pipe("bf16")
    fork_from = torch.cuda.Stream(device=pipe.device)                     # stands for a capture stream: any pool stream
    other = torch.cuda.Stream(device=pipe.device)
    assert other.cuda_stream != fork_from.cuda_stream
    pipe._side_stream, pipe._aux_stream = other, other
    setattr(pipe, which, _second_handle_of(fork_from))
    try:
        with torch.cuda.stream(fork_from):
            pipe._overlap(True)
            handles = {pipe._side_stream.cuda_stream, pipe._aux_stream.cuda_stream}
            assert fork_from.cuda_stream not in handles and len(handles) == 2
            assert pipe.brushnet.side_stream is pipe._side_stream
    finally:
        pipe._overlap(False)
    assert pipe.brushnet.side_stream is None
