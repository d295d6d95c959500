"""Entries whose kernels take a job per grid row, past the 65 535 rows a grid has (`launch_rows`, csrc/common.hpp): the second launch
must start at job 65 535 with every per-job pointer moved on.  tests/test_gpu_hsva.py has this for spng_hsva_batch
(test_a_large_batch_crosses_the_grid_limit); here are the entries that share the launcher and had no such test.  Expected values:
the restatements of tests/test_gpu_alpha.py and tests/tutorial_ref.py."""
import numpy as np
import pytest

import tutorial_ref as tr
from test_gpu_alpha import RGBA, S, restate

pytestmark = pytest.mark.gpu

N = 65537            # one more than the grid-row limit plus one: the smallest count whose second launch has a job behind its first


def test_alpha_and_luminance_batches_cross_the_grid_limit(gpu):
    """one spng_alpha_batch call of N arrays of 3 RGBA<UInt8> pixels, straightened in place, and one spng_luminance_batch call of N
    arrays of 5 pixels to V8: slices of one tensor each; every result reads SPNG_DONE with its own byte and trap counts"""
    s = gpu.load()
    rng = np.random.default_rng(65537)
    px = rng.integers(0, 256, (N * 3, 4), dtype=np.uint8)
    px[rng.random(N * 3) < 0.1, 3] = 0
    want, trapped = restate(px, 8, S)
    # (per array: a component traps where 0 < a < c -- (255 c + a / 2) / a > 255 from c = a + 1 on; held to the restatement's total)
    traps = ((px[:, 3:] > 0) & (px[:, :3] > px[:, 3:])).sum(axis=1).reshape(N, 3).sum(axis=1)
    assert traps.sum() == trapped > N
    d = s.to_device(px.reshape(-1))
    descs = (gpu.AlphaDesc * N)()
    at = d.data_ptr()
    for i in range(N):
        descs[i] = gpu.AlphaDesc(at + 12 * i, at + 12 * i, 3, 8, RGBA, S)
    res = (gpu.Result * N)()
    assert s.lib.spng_alpha_batch(s.ctx, descs, N, None, res) == 0
    assert (d.cpu().numpy().reshape(-1, 4) == want).all()
    got = np.array([(r.status, r.written, r.aux[0]) for r in res])
    assert (got[:, 0] == 0).all() and (got[:, 1] == 12).all() and (got[:, 2] == traps).all()

    px = rng.integers(0, 256, (N * 5, 4), dtype=np.uint8)
    d_in, d_out = s.to_device(px.reshape(-1)), s.to_device(np.full(N * 5, 0xEE, dtype=np.uint8))
    descs = (gpu.LuminanceDesc * N)()
    a, b = d_in.data_ptr(), d_out.data_ptr()
    for i in range(N):
        descs[i] = gpu.LuminanceDesc(a + 20 * i, b + 5 * i, 5, 1)               # (op 1: SPNG_LUMINANCE_V8)
    res = (gpu.Result * N)()
    assert s.lib.spng_luminance_batch(s.ctx, descs, N, None, res) == 0
    assert (d_out.cpu().numpy() == tr.luminance(px)).all()
    got = np.array([(r.status, r.written, r.consumed, r.aux[0]) for r in res])
    assert (got == [0, 5, 20, 0]).all()
