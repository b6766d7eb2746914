"""Helpers of the AP threshold-row tests: the filter that defines a row (NumPy's float32 ``prob >= tau`` on all four
label arrays, then ap_tally.tally), a plain NumPy restatement of the arrays the kernels leave per row (keys ranked over
the whole scene, everything else over the row's points), and small scene builders."""
import numpy as np

F32 = np.float32


def kept_mask(prob, tau):
    return np.asarray(prob, dtype=F32) >= F32(tau)


def filtered(sc, tau):
    """The scene (sem_gt, inst_gt, ps_sem, ps_inst, prob) restricted to the points with prob >= float32(tau)."""
    m = kept_mask(sc[4], tau)
    return [np.asarray(a)[m] for a in sc]


def own_thresholds(scenes, qs=(0.25, 0.5, 1.0)):
    """Thresholds that ARE probabilities of the scenes' points (the q-th of their distinct values, 1.0 = the largest):
    every compare of the row has its equality case."""
    prob = np.unique(np.concatenate([np.asarray(sc[4], dtype=F32) for sc in scenes]))
    return [float(prob[int(q * (len(prob) - 1))]) for q in qs]


def raw_row(sc, mask, max_ps=None, remap=True):
    """What gapro_eval_ap_tables_rows leaves for one scene and one row (the points of ``mask``) ->
    dict(key_code, key_n, ps_n, ps_label, ps_void, ps_sum, pair), pair flat [(K + 1) * (P + 1)]."""
    sem, ins, ps_sem, ps, prob = (np.asarray(a) for a in sc)
    sem, ins, ps_sem, ps = (a.astype(np.int64) for a in (sem, ins, ps_sem, ps))
    if remap:
        sem = np.where(sem != -100, sem - 2, sem)
        sem[(sem == -1) | (sem == -2)] = 18
    inst_ok = (sem >= 0) & (sem < 18) & (ins >= -1)
    code = (sem + 1) * 1000 + ins + 1
    key_code = np.unique(code[inst_ok])           # of the WHOLE scene
    K = len(key_code)
    P = int(max_ps) if max_ps is not None else max(1, int(ps.max(initial=-1)) + 1)
    row = np.where(inst_ok, 1 + np.searchsorted(key_code, code), 0)
    col = np.where(ps == -100, 0, ps + 1)
    m = np.asarray(mask, dtype=bool)
    pair = np.bincount((row * (P + 1) + col)[m], minlength=(K + 1) * (P + 1)).reshape(K + 1, P + 1)
    ps_label = np.zeros(P, np.int64)
    ps_sum = np.zeros(P, np.int64)
    idx = np.flatnonzero(m & (ps != -100))
    for i in idx[::-1]:                           # the first kept point is written last
        ps_label[ps[i]] = ps_sem[i] + 1 if 0 <= ps_sem[i] < 18 else 0
    np.add.at(ps_sum, ps[idx], np.rint(prob[idx].astype(np.float64) * 2.0 ** 32).astype(np.int64))
    return dict(key_code=key_code, key_n=pair[1:].sum(axis=1), ps_n=pair[:, 1:].sum(axis=0), ps_label=ps_label,
                ps_void=pair[0, 1:].copy(), ps_sum=ps_sum, pair=pair.reshape(-1))


def random_scene(seed, n, n_gt, n_ps, classes=17, prob_levels=None):
    """GT id g of class 1 + g % classes, pseudo id mostly g % n_ps with the label p % classes; every GT and pseudo id up
    to the largest is used; some void GT points and some points without a pseudo id.  ``prob_levels``: probabilities
    drawn from these values only (so thresholds can sit ON them), else uniform float32."""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, n_gt, n)
    p = np.where(rng.random(n) < 0.75, g % n_ps, rng.integers(0, n_ps, n))
    g[n - min(n, n_gt):] = np.arange(n_gt - min(n, n_gt), n_gt)
    p[:min(n, n_ps)] = np.arange(min(n, n_ps))
    sem = g % classes + 2
    ps_sem = p % classes
    sem[rng.random(n) < 0.05] = 0
    none = rng.random(n) < 0.1
    none[:min(n, n_ps)] = False
    p[none], ps_sem[none] = -100, -100
    if prob_levels is None:
        prob = rng.random(n).astype(F32)
    else:
        prob = np.asarray(prob_levels, dtype=F32)[rng.integers(0, len(prob_levels), n)]
    return [sem.astype(np.float64), g.astype(np.float64), ps_sem.astype(np.int32), p.astype(np.int32), prob]
