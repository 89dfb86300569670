"""Shared random-LP builders for the tests (seeded, small)."""
import numpy as np

from mvolps_amd.capi import DB, FR, FX, LO, MAX, MIN, UP


def random_general_lp(rng, mmax=9, nmax=10):
    """Feasible-by-construction LP with every bound type on rows and columns."""
    m = int(rng.integers(2, mmax))
    n = int(rng.integers(2, nmax))
    A = np.round(rng.normal(size=(m, n)) * 3)
    A[rng.random((m, n)) < 0.3] = 0
    x0 = rng.integers(0, 4, size=n).astype(float)
    act = A @ x0
    row_b, col_b = [], []
    for i in range(m):
        t = int(rng.choice([LO, UP, DB, FX, FR], p=[0.25, 0.35, 0.2, 0.1, 0.1]))
        l = act[i] - rng.integers(0, 3)
        u = act[i] + rng.integers(0, 3)
        if t == FX:
            l = u = act[i]
        if t == DB and l == u:
            u = l + 1
        row_b.append((t, float(l), float(u)))
    for j in range(n):
        t = int(rng.choice([LO, UP, DB, FX, FR], p=[0.4, 0.1, 0.35, 0.05, 0.1]))
        l = x0[j] - rng.integers(0, 3)
        u = x0[j] + rng.integers(0, 4)
        if t == FX:
            l = u = x0[j]
        if t == DB and l == u:
            u = l + 1
        col_b.append((t, float(l), float(u)))
    c = np.round(rng.normal(size=n) * 5)
    direction = int(rng.choice([MIN, MAX]))
    return A, row_b, col_b, c, direction


def bounds_arrays(bnds):
    lo = np.array([l if t in (LO, DB, FX) else -np.inf for t, l, u in bnds])
    hi = np.array([u if t in (UP, DB) else (l if t == FX else np.inf) for t, l, u in bnds])
    return lo, hi


def load_ilp(api, A, b, c, U):
    from mvolps_amd import synth

    return synth.load_ilp(api, A, b, c, U)


def degenerate_lp(m, n, seed, frac0=0.9):
    """max c x, A x <= b, 0 <= x <= 2, integer data, about 90 % of b equal to zero: the slack basis is a
    massively degenerate vertex on which plain Dantzig pricing stalls (200x300 seed 4 never leaves it)."""
    rng = np.random.default_rng(seed)
    A = rng.integers(-3, 4, size=(m, n)).astype(float)
    b = np.where(rng.random(m) < frac0, 0.0, rng.integers(1, 5, size=m).astype(float))
    c = rng.integers(1, 6, size=n).astype(float)
    return A, b, c


def load_degenerate(api, A, b, c):
    from mvolps_amd.capi import DB, UP
    P = api.create()
    P.load_general(A, [(UP, 0.0, float(x)) for x in b], [(DB, 0.0, 2.0)] * A.shape[1], c)
    return P


# textbook LPs on which Dantzig pricing with lowest-index ties cycles (max c x, A x <= b, x >= 0)
CYCLING = {
    "beale": ([[0.25, -8, -1, 9], [0.5, -12, -0.5, 3], [0, 0, 1, 0]], [0, 0, 1.0], [0.75, -20, 0.5, -6]),
    "chvatal": ([[0.5, -5.5, -2.5, 9], [0.5, -1.5, -0.5, 1], [1, 0, 0, 0]], [0, 0, 1.0], [10, -57, -9, -24.0]),
}


def setcover_ilp(m, n, seed, dens=0.15):
    """min c x, A x >= 1, x binary (A 0/1, every row covered): a MINIMISATION ILP -- bs.cpp bounds and prunes as a
    maximiser whatever the direction (bs.cpp:172,210), so only the repaired mode gets these right."""
    rng = np.random.default_rng(seed)
    A = (rng.random((m, n)) < dens).astype(float)
    for i in range(m):
        if A[i].sum() == 0:
            A[i, rng.integers(n)] = 1.0
    c = rng.integers(1, 10, size=n).astype(float)
    return A, c


def load_setcover(api, A, c):
    from mvolps_amd.capi import DB, IV, LO, MIN
    m, n = A.shape
    P = api.create()
    P.load_general(A, [(LO, 1.0, 0.0)] * m, [(DB, 0.0, 1.0)] * n, c, kinds=[IV] * n, direction=MIN)
    return P


def load_case(api, case):
    """(m, n, seed, U) -> dense_ilp; ("setcover", m, n, seed) -> setcover_ilp"""
    from mvolps_amd import synth
    if case[0] == "setcover":
        return load_setcover(api, *setcover_ilp(*case[1:]))
    A, b, c, U = synth.dense_ilp(*case)
    return load_ilp(api, A, b, c, U)


MILP_FAMILIES = "aaaabbcd"  # sub-family of instance `index`: index % 8 picks the letter, so the shares are fixed


def random_general_milp(seed, index):
    """Instance `index` of the general mixed-integer family: random_general_lp from default_rng(seed + index) plus kinds, a
    constant term and one of four sub-families chosen by the index:

      a  as drawn;
      b  one or two integer columns get half-integer bounds (lb - 0.5, ub + 0.5);
      c  LP-infeasible: two rows that contradict each other (r x >= L and r x <= L - 1);
      d  integer-infeasible with a feasible relaxation: a new integer column z in [-3, 4] and the parity row
         2 x_k + 2 z = 2 x_k(LP start) + 1 on an integer column k that is not fixed.

    Every third index is all-integer, the others have 70 % integer columns.  Every third group of eight is the larger size
    class (up to 20 x 16, at most 8 integer columns, half of its unbounded integer columns boxed) for deeper trees.
    Returns a dict: A, row_b, col_b, c, c0, kinds, direction, family, size_class."""
    from mvolps_amd.capi import CV, IV

    rng = np.random.default_rng(seed + index)
    family = MILP_FAMILIES[index % 8]
    pure = index % 3 == 0
    large = (index // 8) % 3 == 2
    if large:
        A, row_b, col_b, c, direction = random_general_lp(rng, 21, 9 if pure else 17)
    else:
        A, row_b, col_b, c, direction = random_general_lp(rng, 9, 10)
    n = len(c)
    kinds = [IV if (pure or rng.random() < 0.7) else CV for _ in range(n)]
    c0 = float(rng.integers(-3, 4))
    if large:
        ints = [j for j in range(n) if kinds[j] == IV]
        for j in ints[8:]:
            kinds[j] = CV
        for j in ints[:8]:  # an unbounded integer column rarely has a finite LP range at this size: box half of them
            t, l, u = col_b[j]
            if t in (LO, UP, FR) and l < u and rng.random() < 0.5:
                col_b[j] = (DB, l, u)
    ints = [j for j in range(n) if kinds[j] == IV]
    if family == "b" and ints:
        for j in rng.choice(ints, size=min(len(ints), int(rng.integers(1, 3))), replace=False):
            t, l, u = col_b[int(j)]
            col_b[int(j)] = (t, l - 0.5, u + 0.5)
    elif family == "c":
        r = np.round(rng.normal(size=n) * 2)
        r[0] = r[0] or 1.0
        L = float(rng.integers(-3, 4))
        A = np.vstack([A, r, r])
        row_b = row_b + [(LO, L, 0.0), (UP, 0.0, L - 1.0)]
    elif family == "d":
        free = [j for j in ints if col_b[j][0] != FX] or list(range(n))
        k = int(rng.choice(free))
        kinds[k] = IV
        t, l, u = col_b[k]
        start = l if t in (LO, DB, FX) else (u if t == UP else 0.0)
        if t == FX:  # the chosen column has to move for the relaxation to stay feasible
            col_b[k] = (DB, l - 1.0, l + 1.0)
        row = np.zeros(n + 1)
        row[k], row[n] = 2.0, 2.0
        A = np.vstack([np.hstack([A, np.zeros((A.shape[0], 1))]), row])
        row_b = row_b + [(FX, 2.0 * start + 1.0, 2.0 * start + 1.0)]
        col_b = col_b + [(DB, -3.0, 4.0)]
        kinds = kinds + [IV]
        c = np.append(c, 0.0)
    return dict(A=A, row_b=row_b, col_b=col_b, c=c, c0=c0, kinds=kinds, direction=direction, family=family,
                size_class=1 if large else 0)


def milp_arrays(inst):
    """(A, rlo, rhi, clo, chi, c, c0, isint, maximize) of a random_general_milp instance, +-inf where a bound is absent."""
    from mvolps_amd.capi import CV

    rlo, rhi = bounds_arrays(inst["row_b"])
    clo, chi = bounds_arrays(inst["col_b"])
    return (np.asarray(inst["A"], dtype=float), rlo, rhi, clo, chi, np.asarray(inst["c"], dtype=float), float(inst["c0"]),
            np.array([k != CV for k in inst["kinds"]]), inst["direction"] == MAX)


def milp_sha256(inst):
    """Digest of everything the generator produced, so that a change of numpy's stream fails loudly."""
    import hashlib

    A, rlo, rhi, clo, chi, c, c0, isint, maximize = milp_arrays(inst)
    h = hashlib.sha256()
    h.update(repr(A.shape).encode())
    for v in (A, rlo, rhi, clo, chi, c, np.array([c0]), isint.astype(np.float64), np.array([float(maximize)]),
              np.array([float(t) for t, _, _ in inst["row_b"] + inst["col_b"]])):
        h.update(np.ascontiguousarray(v, dtype=np.float64).tobytes())
    return h.hexdigest()


def load_milp(api, inst):
    P = api.create()
    P.load_general(inst["A"], inst["row_b"], inst["col_b"], inst["c"], c0=inst["c0"], kinds=inst["kinds"], direction=inst["direction"])
    return P
