"""A numpy restatement of csrc/perm_tests.h: the energy distance test, the permutation Welch t-test and the Gaussian-kernel MMD
test of one group, with the permutation stream of DESIGN.md §1 "Permutation tests" reproduced bit for bit.

Every statistic is accumulated sequentially in k (MMD: in the documented pair order) and vectorised over the permutations, so it
adds in the order a lane of the kernel does; column 0 of the label matrix is the observed labelling, which goes through the same
arithmetic.  The stream is uint64 arithmetic; the sort is np.argsort(kind="stable")."""
import numpy as np

ENERGY, T_TEST, MMD = 0, 1, 2
TWO_SIDED, LESS, GREATER = 0, 1, 2
CAP = 1462
NAMES = ("statistic", "p_value", "aux", "n_extreme", "n", "n1", "n2", "status")
NAN = float("nan")
U = np.uint64


def draw_labels(seed, n_perm, n, n1):
    """labels[n, n_perm] (bool): row k joins sample 1 in permutation b."""
    out = np.zeros((n, n_perm), bool)
    if n_perm == 0:
        return out
    with np.errstate(over="ignore"):
        state = U(seed) ^ (np.arange(1, n_perm + 1, dtype=U) * U(0xD1B54A32D192ED03))
        taken = np.zeros(n_perm, np.int64)
        for k in range(n):
            state = state + U(0x9E3779B97F4A7C15)
            z = (state ^ (state >> U(30))) * U(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
            z = z ^ (z >> U(31))
            join = (((z >> U(32)) * U(n - k)) >> U(32)) < (n1 - taken).astype(U)
            taken += join
            out[k] = join
    return out


def energy_stats(z, labels, n1):
    n = len(z)
    dn, dn1, dn2 = float(n), float(n1), float(n - n1)
    cols = labels.shape[1]
    a, b, sxx, syy, sxy = (np.zeros(cols) for _ in range(5))
    for k in range(n - 1):
        join = labels[k]
        a = a + np.where(join, 1.0, 0.0)
        b = b + np.where(join, 0.0, 1.0)
        d, ra, rb = z[k + 1] - z[k], dn1 - a, dn2 - b
        sxx = sxx + d * (a * ra)
        syy = syy + d * (b * rb)
        sxy = sxy + d * (a * rb + b * ra)
    return (dn1 * dn2 / dn) * (2.0 * sxy / (dn1 * dn2) - (2.0 * sxx / (dn1 * dn1) + 2.0 * syy / (dn2 * dn2)))


def t_stats(z, labels, n1):
    """-> (t, df) per labelling."""
    n = len(z)
    dn1, dn2 = float(n1), float(n - n1)
    c = z - z[n // 2]
    cols = labels.shape[1]
    s1, q1, s2, q2 = (np.zeros(cols) for _ in range(4))
    for k in range(n):
        join, ck, cc = labels[k], c[k], c[k] * c[k]
        s1 = s1 + np.where(join, ck, 0.0)
        q1 = q1 + np.where(join, cc, 0.0)
        s2 = s2 + np.where(join, 0.0, ck)
        q2 = q2 + np.where(join, 0.0, cc)
    m1, m2 = s1 / dn1, s2 / dn2
    e1, e2 = (q1 - s1 * m1) / (dn1 - 1.0) / dn1, (q2 - s2 * m2) / (dn2 - 1.0) / dn2
    se2 = e1 + e2
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = se2 > 0.0
        t = np.where(ok, (m1 - m2) / np.sqrt(np.where(ok, se2, 1.0)), NAN)
        df = np.where(ok, se2 * se2 / (e1 * e1 / (dn1 - 1.0) + e2 * e2 / (dn2 - 1.0)), NAN)
    return t, df


def median_sigma(z):
    """The lower median of the pairwise distances of the sorted z: one order statistic."""
    n = len(z)
    i, j = np.triu_indices(n, 1)
    d = z[j] - z[i]
    want = (len(d) + 1) // 2
    return float(np.partition(d, want - 1)[want - 1])


def pair_order(i, n):
    """The j of row i in the kernel's order: blocks of 64 columns ascending from the one that holds i, within a block descending."""
    js = [np.arange(min(j0 + 63, n - 1), max(j0, i + 1) - 1, -1) for j0 in range(i // 64 * 64, n, 64)]
    return np.concatenate(js)


def mmd_stats(z, labels, n1, sigma):
    n = len(z)
    dn1, dn2 = float(n1), float(n - n1)
    den = 2.0 * sigma * sigma
    cols = labels.shape[1]
    sxx, syy, sxy = (np.zeros((1, cols)) for _ in range(3))
    for i in range(n - 1):
        js = pair_order(i, n)
        d = z[i] - z[js]
        kv = np.exp(-(d * d) / den)[:, None]
        bi, bj = labels[i][None, :], labels[js]
        # (ufunc.accumulate adds strictly in sequence: the carry, then the row's pairs in their order)
        sxx = np.add.accumulate(np.vstack([sxx, np.where(bi & bj, kv, 0.0)]), axis=0)[-1:]
        syy = np.add.accumulate(np.vstack([syy, np.where(~bi & ~bj, kv, 0.0)]), axis=0)[-1:]
        sxy = np.add.accumulate(np.vstack([sxy, np.where(bi != bj, kv, 0.0)]), axis=0)[-1:]
    sxx, syy, sxy = sxx[0], syy[0], sxy[0]
    return ((dn1 + 2.0 * sxx) / (dn1 * dn1) + (dn2 + 2.0 * syy) / (dn2 * dn2)) - 2.0 * sxy / (dn1 * dn2)


def group_stats(v, sample, test, n_perm=1000, seed=0, sigma=NAN, cap=CAP):
    """-> (counts (n, n1, n2), status, aux, the statistics [1 + n_perm] with the observed one first, or None)."""
    v = np.asarray(v, np.float64)
    ok = ~np.isnan(v)
    x, first = v[ok], np.asarray(sample)[ok] == 0
    n, n1 = len(x), int(first.sum())
    counts = (n, n1, n - n1)
    if np.isinf(x).any() or n1 < 2 or n - n1 < 2:
        return counts, 6, NAN, None
    if test == MMD and len(v) > cap:
        return counts, 7, NAN, None
    order = np.argsort(x, kind="stable")
    z, obs = x[order], first[order]
    aux = NAN
    if test == MMD:
        aux = float(sigma) if sigma > 0.0 else median_sigma(z)
        if not aux > 0.0:
            return counts, 0, aux, np.full(1, NAN)
    labels = np.concatenate([obs[:, None], draw_labels(seed, n_perm, n, n1)], axis=1)
    if test == ENERGY:
        stats = energy_stats(z, labels, n1)
    elif test == T_TEST:
        stats, df = t_stats(z, labels, n1)
        aux = float(df[0])
    else:
        stats = mmd_stats(z, labels, n1, aux)
    return counts, 0, aux, stats


def extreme(stats, test, alternative):
    """The permutations that count against the observed statistic (stats[0])."""
    obs, perm = stats[0], stats[1:]
    with np.errstate(invalid="ignore"):
        if test != T_TEST or alternative == GREATER:
            return perm >= obs
        if alternative == LESS:
            return perm <= obs
        return np.abs(perm) >= abs(obs)


def group_record(v, sample, test, alternative=TWO_SIDED, n_perm=1000, seed=0, sigma=NAN, cap=CAP):
    counts, status, aux, stats = group_stats(v, sample, test, n_perm, seed, sigma, cap)
    rec = np.full(8, NAN)
    rec[4:7] = counts
    rec[7] = status
    if status:
        return rec
    obs = stats[0]
    n_extreme = 0 if obs != obs else int(extreme(stats, test, alternative).sum())
    rec[0], rec[2], rec[3] = obs, aux, n_extreme
    if obs == obs and n_perm > 0:
        rec[1] = (1.0 + n_extreme) / (n_perm + 1.0)
    return rec


def reference(off, v, sample, test, alternative=TWO_SIDED, n_perm=1000, seed=0, sigma=NAN, cap=CAP):
    """records[G, 8] of a call; a group of more than `cap` rows is on the large path (MMD: status 7)."""
    return np.array([group_record(v[off[g]:off[g + 1]], sample[off[g]:off[g + 1]], test, alternative, n_perm, seed, sigma, cap)
                     for g in range(len(off) - 1)]).reshape(-1, 8)


def make_group(rng, n, n1=None, ties=0.0, nan_share=0.0, shift=0.6):
    """A drawn group: n valid rows (n1 of them sample 0 and shifted, in a drawn order) with a share of NaN rows between them; ties > 0
    rounds the values to integers of a range that makes about that share of the rows tied."""
    n1 = int(rng.integers(2, n - 1)) if n1 is None else n1
    v = rng.normal(size=n) + shift * (np.arange(n) < n1)
    if ties > 0.0:
        v = np.round(v * max(1.0, (1.0 - ties) * n / 4.0))
    s = np.where(np.arange(n) < n1, 0, rng.integers(1, 4, size=n)).astype(np.int32)
    p = rng.permutation(n)
    v, s = v[p], s[p]
    extra = int(round(nan_share * n))
    if extra:
        at = np.sort(rng.integers(0, n + 1, size=extra))
        v, s = np.insert(v, at, np.nan), np.insert(s, at, rng.integers(0, 2, size=extra).astype(np.int32))
    return v, s


def pack(groups):
    """-> (off, v, sample) of a list of (v, sample) groups."""
    off = np.concatenate([[0], np.cumsum([len(g[0]) for g in groups])]).astype(np.int64)
    v = np.concatenate([g[0] for g in groups]) if groups else np.zeros(0)
    s = np.concatenate([g[1] for g in groups]).astype(np.int32) if groups else np.zeros(0, np.int32)
    return off, np.asarray(v, np.float64), s
