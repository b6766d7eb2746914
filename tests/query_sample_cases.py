"""The cases of the query-sampling tests (tests/test_query_sample_cpu.py, tests/test_query_sample_gpu.py): the smallest
shapes at which gapro_fps_batch and gapro_ball_query_batch can go wrong, each milliseconds of GPU work.  A case is a
dict; ``form`` says which public function takes it:

``fps`` / ``ball``             the batch-flat functions: xyz f32[n, 3], offset, new_offset (int32 or int64)
``fps_batched`` / ``ball_batched``  pointnet2's: xyz f32[B, N, 3] (the near-origin skip applies to ``fps_batched``)

``flags`` are the status bits the case must raise (0: none).
"""
import numpy as np

F = np.float32


def _rand(seed, n, scale=4.0):
    return (np.random.default_rng(seed).random((n, 3)) * scale).astype(F)


def lattice(k=6, step=0.25):
    g = np.arange(k, dtype=F) * F(step)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(F)


def _fps(xyz, sizes, outs, dtype=np.int32, leading_zero=False, flags=0):
    off, new = np.cumsum(sizes), np.cumsum(outs)
    if leading_zero:
        off, new = np.concatenate([[0], off]), np.concatenate([[0], new])
    return dict(form="fps", xyz=np.ascontiguousarray(xyz, F), offset=off.astype(dtype), new_offset=new.astype(dtype),
                flags=flags)


def _mag(p):
    x, y, z = (F(v) for v in p)
    return F(F(F(x * x) + F(y * y)) + F(z * z))


def on_the_origin_ball():
    """Two points (x, 0.02, 0): the first has the float32 magnitude ((x*x + y*y) + z*z) == float32(1e-3) exactly, so it
    lies ON the ball and is skipped; the second is the next x whose magnitude exceeds it, the nearest candidate."""
    y = F(0.02)
    x = np.sqrt(np.float64(1e-3) - np.float64(y) ** 2).astype(F)
    for _ in range(4096):
        x = np.nextafter(x, F(0), dtype=F)
    on = None
    for _ in range(8192):
        m = _mag((x, y, 0))
        if m == F(1e-3):
            on = x
        elif m > F(1e-3) and on is not None:
            return (on, y, F(0)), (x, y, F(0))
        x = np.nextafter(x, F(1), dtype=F)
    raise AssertionError("no float32 point with the magnitude float32(1e-3)")


def fps_cases(xyz_capacity, capacity):
    out = {}
    # sample sizes at the wave and workgroup edges, each with m = 1, 2, n and n + 3 (repeats) in one batch
    for n in (1, 2, 63, 64, 65, 1023, 1024, 1025):
        out["size_%d" % n] = _fps(_rand(n, 4 * n), [n] * 4, [1, 2, n, n + 3])
    # the edges of the three paths: m <= 8
    for name, n in (("xyz_capacity", xyz_capacity), ("xyz_capacity_plus_1", xyz_capacity + 1), ("capacity", capacity),
                    ("capacity_plus_1", capacity + 1)):
        out[name] = _fps(_rand(n, n, 10.0), [n], [8])
    # the three paths in one call
    sizes = [5, capacity + 1, xyz_capacity + 1, 70]
    out["paths_mixed"] = _fps(_rand(11, sum(sizes), 10.0), sizes, [4, 5, 6, 7], dtype=np.int64)
    # exact arithmetic and plenty of ties: the tie rule decides from the third sample on
    lat = lattice()
    out["lattice"] = _fps(lat, [len(lat)], [40])
    out["lattice_shuffled"] = _fps(lat[np.random.default_rng(5).permutation(len(lat))], [len(lat)], [40])
    # no exact arithmetic and no ties: the rounding of the distance decides the bits of the minima
    out["random_5000"] = _fps(_rand(7, 5000, 1.0), [5000], [256])
    dup = np.repeat(_rand(8, 50), 3, axis=0)
    out["duplicates"] = _fps(dup, [150], [60])
    # batches
    pts = _rand(9, 300)
    out["batch3"] = _fps(pts, [100, 130, 70], [10, 12, 9])
    out["batch3_leading_zero"] = _fps(pts, [100, 130, 70], [10, 12, 9], leading_zero=True)
    out["batch3_int64"] = _fps(pts, [100, 130, 70], [10, 12, 9], dtype=np.int64)
    out["empty_middle"] = _fps(pts[:170], [100, 0, 70], [10, 0, 9])
    out["no_points"] = _fps(pts[:170], [100, 0, 70], [10, 3, 9], flags=2)
    nan = pts.copy()
    nan[150, 1] = np.nan
    out["nan_coordinate"] = _fps(nan, [100, 130, 70], [10, 12, 9], flags=4)
    inf = pts.copy()
    inf[0, 0] = np.inf
    out["inf_first_point"] = _fps(inf, [100, 130, 70], [10, 12, 9], flags=4)
    out["offsets_decrease"] = dict(form="fps", xyz=pts, offset=np.array([100, 90, 300], np.int32),
                                   new_offset=np.array([10, 22, 31], np.int32), flags=1)
    out["offsets_beyond"] = dict(form="fps", xyz=pts, offset=np.array([100, 230, 301], np.int32),
                                 new_offset=np.array([10, 22, 31], np.int32), flags=1)
    # pointnet2's near-origin skip: points inside, on and outside the 1e-3 ball; a sample with every point inside
    on, outside = on_the_origin_ball()
    a = _rand(10, 70, 2.0)
    a[0] = (0.01, 0.0, 0.0)  # inside, and the first output all the same
    a[3] = on                # on the ball: skipped
    a[5] = outside           # the first float32 outside: a candidate
    a[7] = (0.0, 0.02, 0.01)  # inside
    inside = (_rand(12, 70, 1.0) * F(0.015)).astype(F)
    out["skip_origin"] = dict(form="fps_batched", xyz=np.stack([a, inside]), npoint=12, flags=0)
    out["batched_no_skip_needed"] = dict(form="fps_batched", xyz=(_rand(13, 130, 3.0) + F(1)).reshape(2, 65, 3),
                                         npoint=9, flags=0)
    return out


def _line(hit_positions, n, far=5.0):
    """n points on the x axis: those at ``hit_positions`` within 0.5 of the origin, the others at ``far``."""
    p = np.zeros((n, 3), F)
    p[:, 0] = far
    hit_positions = np.asarray(hit_positions, np.int64)
    p[hit_positions, 0] = (0.4 * np.arange(len(hit_positions)) / max(len(hit_positions), 1)).astype(F)
    return p


def _ball(xyz, new_xyz, sizes, queries, radius, nsample, dtype=np.int32, leading_zero=False, flags=0):
    off, new = np.cumsum(sizes), np.cumsum(queries)
    if leading_zero:
        off, new = np.concatenate([[0], off]), np.concatenate([[0], new])
    return dict(form="ball", xyz=np.ascontiguousarray(xyz, F), new_xyz=np.ascontiguousarray(new_xyz, F),
                offset=off.astype(dtype), new_offset=new.astype(dtype), radius=radius, nsample=nsample, flags=flags)


def ball_cases():
    out = {}
    origin = np.zeros((1, 3), F)
    for ns in (1, 32, 64):
        for extra in (-1, 0, 1):  # nsample - 1, nsample and nsample + 1 hits, spread over 300 scan positions
            hits = np.random.default_rng(100 * ns + extra + 1).choice(300, ns + extra, replace=False)
            out["ns%d_hits%+d" % (ns, extra)] = _ball(_line(np.sort(hits), 300), origin, [300], [1], 0.5, ns)
    out["hits_at_63_and_64"] = _ball(_line([63, 64], 130), origin, [130], [1], 0.5, 4)
    out["hits_at_255_and_256"] = _ball(_line([255, 256, 299], 300), origin, [300], [1], 0.5, 4)
    out["early_stop_in_first_chunk"] = _ball(_line([2, 9, 40, 41, 60, 63, 64, 100, 290], 300), origin, [300], [1], 0.5, 3)
    out["stop_at_the_last_point"] = _ball(_line([10, 299], 300), origin, [300], [1], 0.5, 2)
    out["radius_zero"] = _ball(_rand(20, 100), _rand(20, 100)[:5], [100], [5], 0.0, 8)
    lat = np.stack(np.meshgrid(*[np.arange(5, dtype=F) * F(0.25)] * 3, indexing="ij"), -1).reshape(-1, 3)
    out["lattice_exactly_r"] = _ball(lat, lat, [len(lat)], [len(lat)], 0.5, 32)  # distance 0.5 exactly: excluded
    # two adjacent samples whose boundary points lie within r of each other: no leak either way
    a, b = _rand(21, 80, 1.0), _rand(22, 90, 1.0)
    b[0] = a[-1] + F(0.01)
    both = np.concatenate([a, b])
    out["no_leak"] = _ball(both, both, [80, 90], [80, 90], 0.3, 16)
    out["no_leak_leading_zero_int64"] = _ball(both, both, [80, 90], [80, 90], 0.3, 16, dtype=np.int64,
                                              leading_zero=True)
    out["sample_of_one_point"] = _ball(both[:81], both[[0, 80, 80]] + F(0.001), [80, 1], [1, 2], 0.3, 4)
    out["empty_sample_of_queries"] = _ball(both, both[:6], [80, 0, 90], [2, 2, 2], 5.0, 4)
    out["offsets_decrease"] = dict(form="ball", xyz=both, new_xyz=both[:6], offset=np.array([80, 70, 170], np.int32),
                                   new_offset=np.array([2, 4, 6], np.int32), radius=5.0, nsample=4, flags=1)
    out["queries_beyond_the_offsets"] = dict(form="ball", xyz=both, new_xyz=both[:6],
                                             offset=np.array([80, 170], np.int32),
                                             new_offset=np.array([2, 4], np.int32), radius=5.0, nsample=4, flags=1)
    pts = _rand(23, 130, 1.0).reshape(2, 65, 3)
    out["batched"] = dict(form="ball_batched", xyz=pts, new_xyz=np.ascontiguousarray(pts[:, [0, 33, 64]]), radius=0.4,
                          nsample=32, flags=0)
    return out


def sample_queries_case():
    sizes = [301, 287]
    return dict(locs=_rand(30, sum(sizes), 1.5), batch_offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32),
                batch_size=2, n_sample=16, radius=0.2, n_neighbor=32, n_neighbor_post=8)
