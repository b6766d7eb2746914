"""Inputs of the exact-sum helper tests (test_exact_sum_cpu.py / test_exact_sum_gpu.py) and the call both share:
gapro_debug_exact_sum evaluates csrc/exact_sum.h's fixed_point_shift, to_fixed and fixed_mean elementwise, on the host
(no context) or in one workgroup on the device."""
import ctypes as C

import numpy as np

FLT_MIN, FLT_MAX = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)
FLT_SUBNORMAL, DBL_SUBNORMAL = float(np.float32(1e-45)), 5e-324  # the smallest float32 / float64 subnormals

SHIFT_ABSMAX = (0.0, -0.0, FLT_SUBNORMAL, DBL_SUBNORMAL, FLT_MIN, float(np.float32(0.99999994)), 1.0, 255.0, FLT_MAX,
                1e300, float("inf"), float("nan"))
SHIFT_N = (1, 2, 3, 4, 5, 1023, 1024, 1025, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, 1 << 40, 1 << 62)
SHIFT_KNOWN = ((1.0, 1024, 50), (1e-45, 1, 210), (1e300, 1 << 40, -976))


def shift_inputs():
    """(absmax f64[], n i64[]): SHIFT_ABSMAX x SHIFT_N, then the three pairs whose shift the spec states."""
    a = [x for x in SHIFT_ABSMAX for _ in SHIFT_N] + [k[0] for k in SHIFT_KNOWN]
    n = [m for _ in SHIFT_ABSMAX for m in SHIFT_N] + [k[1] for k in SHIFT_KNOWN]
    return np.array(a, np.float64), np.array(n, np.int64)


def fixed_inputs():
    """(x f64[], k i32[]): ties at several scales (they round to even), negative values, and the largest terms the rule
    admits: |x| just below 2^e at k = 61 - e, n = 1."""
    x, k = [], []
    for s in (0, 10, -3, 50, 61, -67):
        for t in (0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, 0.49999999999999994, 1.0, -1.0, 0.0):
            x.append(float(np.ldexp(t, -s)))
            k.append(s)
    for v, s in ((-3.7, 20), (-1e-3, 40), (-255.0, 30), (-FLT_MAX, -67), (-FLT_SUBNORMAL, 150), (-0.1, 0)):
        x.append(v)
        k.append(s)
    for v in (FLT_MAX, 255.0, 1.0, float(np.float32(0.99999994)), float(np.nextafter(1.0, 0.0)), FLT_MIN, FLT_SUBNORMAL,
              1e300):
        e = int(np.frexp(v)[1])
        x += [v, -v]
        k += [61 - e, 61 - e]
    return np.array(x, np.float64), np.array(k, np.int32)


def mean_inputs():
    """(sum i64[], k i32[], count f64[]): sums near +-2^61 and small ones, at several scales, counts 1, 3 and 2^24 + 1."""
    big = 1 << 61
    sums = (big - 1, -(big - 1), big - 256, -(big - 256), big - 257, (1 << 53) + 1, -((1 << 53) + 1), 7, -7, 1, 0)
    s, k, c = [], [], []
    for v in sums:
        for sh in (61, 50, 0, -67, 210):
            for cnt in (1.0, 3.0, float((1 << 24) + 1)):
                s.append(v)
                k.append(sh)
                c.append(cnt)
    return np.array(s, np.int64), np.array(k, np.int32), np.array(c, np.float64)


def evaluate(ctx=None):
    """(shift i32[], fixed i64[], mean f64[]) of the three input groups: ctx None = the host leg, a gapro_amd._lib
    Context = the device leg (one launch of one workgroup)."""
    from gapro_amd import _lib

    dbg = _lib.load_debug()
    a, n = shift_inputs()
    x, xk = fixed_inputs()
    s, mk, cnt = mean_inputs()
    ins = [a, n, x, xk, s, mk, cnt]
    outs = [np.full(len(a), -12345, np.int32), np.full(len(x), -12345, np.int64), np.full(len(s), -12345.0, np.float64)]
    if ctx is None:
        ptr = lambda v: C.c_void_p(v.ctypes.data)
        rc = dbg.gapro_debug_exact_sum(None, None, len(a), ptr(a), ptr(n), ptr(outs[0]), len(x), ptr(x), ptr(xk),
                                       ptr(outs[1]), len(s), ptr(s), ptr(mk), ptr(cnt), ptr(outs[2]))
        assert rc == 0
        return outs
    import torch

    d_in = [torch.from_numpy(v).cuda() for v in ins]
    d_out = [torch.from_numpy(v).cuda() for v in outs]
    ptr = lambda t: C.c_void_p(t.data_ptr())
    ctx.check(dbg.gapro_debug_exact_sum(ctx.handle, None, len(a), ptr(d_in[0]), ptr(d_in[1]), ptr(d_out[0]), len(x),
                                        ptr(d_in[2]), ptr(d_in[3]), ptr(d_out[1]), len(s), ptr(d_in[4]), ptr(d_in[5]),
                                        ptr(d_in[6]), ptr(d_out[2])))
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in d_out]
