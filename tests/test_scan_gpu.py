"""csrc/scan.h's device-wide exclusive scan on the MI355X, through gapro_debug_scan: exact equality with numpy.cumsum
and total == sum, at the edges of its three launches.

Sizes: the wave (64), the workgroup (256) and the 1024-item block of k_devscan_sums / k_devscan_apply, each with its
neighbours; 2049 (a third, one-item block); 262 144 = 256 blocks, the last size k_devscan_carry does in one trip of its
loop; 262 145, the first with a second trip (the running carry); 525 313 = 2 * 262 144 + 1025, a third trip that ends in
a partial block.  Values: zeros, ones, seeded 0/1 flags (what voxelize.hip and spconv.hip scan) and seeded counts in
[0, 4096] (the range of spp_pool.hip's histogram cells), the counts also in place, as spp_pool.hip scans them.  Every
case runs twice and the two results are compared byte for byte."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 262143, 262144, 262145, 525313)
KINDS = ("zeros", "ones", "flags", "counts", "counts_in_place")
SCAN_BLOCK = 1024  # csrc/scan.h kScanBlock


def _values(kind, n):
    rng = np.random.default_rng(n)
    if kind == "zeros":
        return np.zeros(n, np.int32)
    if kind == "ones":
        return np.ones(n, np.int32)
    if kind == "flags":
        return rng.integers(0, 2, size=n).astype(np.int32)
    return rng.integers(0, 4097, size=n).astype(np.int32)


def _scan(v, in_place):
    """(exclusive scan int32[n], total) of one call of gapro_debug_scan on fresh device arrays."""
    import torch
    from gapro_amd._lib import Context

    ctx = Context.get(0)
    n = len(v)
    d_in = torch.from_numpy(v).cuda()
    d_out = d_in if in_place else torch.full((n,), -12345, dtype=torch.int32, device="cuda")
    d_sums = torch.full((-(-n // SCAN_BLOCK),), -12345, dtype=torch.int32, device="cuda")
    d_total = torch.full((1,), -12345, dtype=torch.int32, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())
    torch.cuda.synchronize()
    ctx.check(ctx.dbg.gapro_debug_scan(ctx.handle, None, n, ptr(d_in), ptr(d_out), ptr(d_sums), ptr(d_total)))
    torch.cuda.synchronize()
    if not in_place:
        assert (d_in.cpu().numpy() == v).all()  # the input is only read
    return d_out.cpu().numpy(), int(d_total.cpu()[0])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_scan_equals_cumsum(n, kind):
    v = _values(kind, n)
    inclusive = np.cumsum(v, dtype=np.int64)
    assert inclusive[-1] < 2 ** 31
    want = (inclusive - v).astype(np.int32)
    got, total = _scan(v, kind == "counts_in_place")
    assert got.dtype == np.int32 and got.shape == (n,)
    np.testing.assert_array_equal(got, want)
    assert total == int(inclusive[-1])
    again, total_again = _scan(v, kind == "counts_in_place")
    assert again.tobytes() == got.tobytes() and total_again == total
