"""Cases for the three wave-cooperative derivative launches on mixed work lists (device/gradcoop.hip k_mala_grad, h2hess.hip k_h2_hess, h2gauss.hip
k_h2_gauss; the list machinery they share: device/dh2coop.h; probes: include/lmc_abi.h lmc_*_list_probe).  What the launches compute is tested elsewhere;
these cases exercise how they FIND their work: 336 bins (42 techniques x 8 material signatures) of one items array, a task table every block rebuilds, a
bisection per task, a grid-stride loop that walks the tasks in reversed order and reuses one LDS staging area.  A chain's output row must not depend on
any of it, so every check on the device is bit equality with the same state's row from the simplest launch (tests/test_gpu_coop_lists.py).

The states of the gradient and the Hessian launch come from tests/golden/derv_vectors_full.npz (271 full-material states, 46 (scene, c, l) groups); a
bin is brought to a wanted population by replicating the technique's states cyclically.  The Gaussian launch needs no scene: its inputs are the synthetic
Hessians of tests/h2_refs.py.  Plain NumPy, deterministic.  tests/test_coop_cases.py checks without a GPU that every case obeys the probes' validity
rules and covers the edges it claims."""
import os

import numpy as np

from tests import h2_refs

NSIG, NTECH, BINS = 8, 42, 336  # dh2coop.h H2_NSIG, H2_NTECH, H2_NBINS
UNTOUCHED_BITS = 0x7FC0BEEF  # what a probe's float output holds where the launch wrote nothing
F_GSEL = 64  # dchain.h: the chain's current Gaussian is in the second buffer
VERT_WORDS = 592  # include/lmc_abi.h LMC_PROBE_VERT_WORDS
KERNELS = ("mala_grad", "h2_hess", "h2_gauss")  # index = the `kernel` argument of lmc_coop_plan_probe
MG_LDS_WORDS, HESS_LDS_WORDS = 4352, 3328  # LDS words of records per wave (gradcoop.hip, h2hess.hip)
H2K_DENSE, H2K_ISO_EARLYOUT = 0, 1
GRAD_ROW, HESS_ROW, GAUSS_ROW = 32, 288, 544  # words per chain of the three outputs
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "derv_vectors_full.npz")
GRID_MAX = 4096
POPULATION_KINDS = ("one", "ipw-1", "ipw", "ipw+1", "2ipw", "2ipw+1")
SIGMA = 0.01


# ------------------------------------------------------------------------------------------------ the documented plan, restated
def tech_index(c, l):
    """dh2coop.h H2TechIndex: the derivative programs exist for 1 <= c <= 9, 0 <= l <= 8, 3 <= c + l <= 9; -1 = no program"""
    s = c + l
    if c < 1 or c > 9 or l < 0 or l > 8 or s < 3 or s > 9:
        return -1
    return (s - 1) * s // 2 - 3 + l


def tech_of(t):
    s, base = 3, 0
    while base + s <= t:
        base, s = base + s, s + 1
    return s - (t - base), t - base  # (c, l)


def tech_dim(t):
    c, l = tech_of(t)
    return 2 * (c + l - 1)


def rec_words(t):
    """words of a state's record a wave stages: (c, l) header at 20 words, 238 + 59 (c + l - 3) vertParams, padded to four"""
    c, l = tech_of(t)
    return (20 + 238 + 59 * (c + l - 3) + 3) & ~3


def blocks_of_dim(dim):
    return (dim // 2) * (dim // 2 + 1) // 2


def plan(kernel, t):
    """(states per task, what bounds it: "lanes", "lds", "tie" or "fixed") of technique t -- the documented formulas:
    gradient min(64 / (dim / 2), 4352 / recWords), Hessian min(64 / blocks(dim), 3328 / recWords), Gaussian 4"""
    if kernel == "h2_gauss":
        return 4, "fixed"
    dim = tech_dim(t)
    by_lanes = 64 // (dim // 2) if kernel == "mala_grad" else 64 // blocks_of_dim(dim)
    by_lds = (MG_LDS_WORDS if kernel == "mala_grad" else HESS_LDS_WORDS) // rec_words(t)
    return min(by_lanes, by_lds), "tie" if by_lanes == by_lds else "lanes" if by_lanes < by_lds else "lds"


def ipw(kernel, t):
    return plan(kernel, t)[0]


def population(kind, n):
    return {"one": 1, "ipw-1": n - 1, "ipw": n, "ipw+1": n + 1, "2ipw": 2 * n, "2ipw+1": 2 * n + 1}[kind]


def total_tasks(kernel, count):
    return sum((int(count[b]) + ipw(kernel, b // NSIG) - 1) // ipw(kernel, b // NSIG) for b in range(BINS))


def grid_sizes(tasks):
    return (1, 2, 3, tasks - 1, tasks, 1024)


# ------------------------------------------------------------------------------------------------ the golden states
_golden = None


def golden():
    """The golden file as a dict of arrays, plus tech[i] = technique index of state i"""
    global _golden
    if _golden is None:
        z = dict(np.load(GOLDEN))
        z["tech"] = np.array([tech_index(int(c), int(l)) for c, l in zip(z["c"], z["l"])])
        _golden = z
    return _golden


def scene_techs(sid):
    z = golden()
    return sorted(set(int(t) for t in z["tech"][z["scene_id"] == sid]))


def states_of(sid, t):
    z = golden()
    return np.flatnonzero((z["scene_id"] == sid) & (z["tech"] == t))


# ------------------------------------------------------------------------------------------------ work lists
class Case:
    """One launch: src[N] = the pool state every chain's record is a copy of (listed or not), the work list (items, count, start) and the grid"""

    def __init__(self, name, kernel, src, items, count, start, grid_blocks, scene=None, **extra):
        self.name, self.kernel, self.scene = name, kernel, scene
        self.src, self.items = np.asarray(src, np.int64), np.asarray(items, np.int32)
        self.count, self.start, self.grid_blocks = np.asarray(count, np.int32), np.asarray(start, np.int32), int(grid_blocks)
        self.N, self.n_list = len(self.src), len(self.items)
        self.listed = np.zeros(self.N, bool)
        self.listed[self.items[self.items_in_bins()]] = True
        self.__dict__.update(extra)

    def items_in_bins(self):
        """positions of `items` that some bin lists"""
        pos = [np.arange(self.start[b], self.start[b] + self.count[b]) for b in range(BINS) if self.count[b]]
        return np.concatenate(pos) if pos else np.zeros(0, np.int64)

    def bin_of_chain(self):
        out = np.full(self.N, -1)
        for b in range(BINS):
            out[self.items[self.start[b]: self.start[b] + self.count[b]]] = b
        return out

    def with_grid(self, grid_blocks):
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.grid_blocks, c.name = int(grid_blocks), "%s/grid%d" % (self.name, grid_blocks)
        return c


def _lay_out(pops, pool_of_bin, unlisted_pool, seed, spare=True):
    """pops: bin -> population.  The bins appear in `items` in bin order and start[] is the exclusive prefix of count[] over ALL bins, as LaunchBinsCompact
    leaves them; the chain ids are a random subset of [0, N) in random order (N about twice the list, the unlisted chains in between hold valid states
    too); a bin's states are its pool's, taken cyclically from a random first one -- so a population beyond the pool replicates states."""
    rng = np.random.default_rng(seed)
    n_list = int(sum(pops.values()))
    N = 2 * n_list + 1 if spare else n_list
    ids = rng.permutation(N)[:n_list] if spare else np.arange(n_list)
    src = np.asarray(unlisted_pool)[rng.integers(0, len(unlisted_pool), N)]
    count, start, pos = np.zeros(BINS, np.int32), np.zeros(BINS, np.int32), 0
    for b in range(BINS):
        start[b] = pos
        p = int(pops.get(b, 0))
        if p:
            pool = pool_of_bin(b)
            first = int(rng.integers(0, len(pool))) if spare else 0
            src[ids[pos: pos + p]] = [pool[(first + k) % len(pool)] for k in range(p)]
            count[b], pos = p, pos + p
    return src, ids.astype(np.int32), count, start


def _sid_pool(sid):
    return np.flatnonzero(golden()["scene_id"] == sid)


def baseline_case(kernel, sid, t):
    """the simplest launch, the one the existing probes make: the technique's golden states in its signature-0 bin, identity order, nobody unlisted"""
    st = states_of(sid, t)
    src, items, count, start = _lay_out({t * NSIG: len(st)}, lambda b: st, st, 0, spare=False)
    start[:] = 0  # (the existing probes leave start at zero everywhere)
    return Case("baseline/%s/s%d/t%d" % (kernel, sid, t), kernel, src, items, count, start, 1024, scene=sid)


def count_edge_case(kernel, sid, kind):
    """every technique of the scene in one launch, each in ONE bin (its signature moves with the technique) of population `kind` relative to the
    technique's own states per task -- 0 ("ipw-1" where a task takes one state) leaves that technique out: an empty bin between full ones"""
    k = POPULATION_KINDS.index(kind)
    pops = {t * NSIG + (t + k) % NSIG: population(kind, ipw(kernel, t)) for t in scene_techs(sid)}
    src, items, count, start = _lay_out(pops, lambda b: states_of(sid, b // NSIG), _sid_pool(sid), 1000 * sid + k)
    return Case("count/%s/s%d/%s" % (kernel, sid, kind), kernel, src, items, count, start, 1024, scene=sid)


def _mixed_pops(kernel, techs):
    """all eight signature bins of every technique: six of one state, one of two, one of a full task and a state"""
    pops = {}
    for t in techs:
        pattern = [1, 1, ipw(kernel, t) + 1, 1, 1, 2, 1, 1]
        for s in range(NSIG):
            pops[t * NSIG + s] = pattern[(s + t) % NSIG]
    return pops


def mixed_case(kernel, sid, grid_blocks=1024):
    """all techniques of one scene (the scene block is a launch argument) over all their bins, chain ids shuffled within and across bins"""
    src, items, count, start = _lay_out(_mixed_pops(kernel, scene_techs(sid)), lambda b: states_of(sid, b // NSIG), _sid_pool(sid), 77 + sid)
    return Case("mixed/%s/s%d" % (kernel, sid), kernel, src, items, count, start, grid_blocks, scene=sid)


def empty_case(case):
    """the stage with no takers: the same chains and items, every count zero"""
    c = case.with_grid(case.grid_blocks)
    c.count, c.start, c.name = np.zeros(BINS, np.int32), np.zeros(BINS, np.int32), case.name + "/empty"
    c.listed = np.zeros(c.N, bool)
    return c


def record_inputs(case):
    """the arrays lmc_mala_grad_list_probe / lmc_h2_hess_list_probe take for a case: primary [N, 17], c[N], l[N], vert [N, 592], scene38"""
    z = golden()
    vert = np.zeros((case.N, VERT_WORDS), np.float32)
    vert[:] = z["vert"][case.src][:, :VERT_WORDS]
    return z["primary"][case.src].astype(np.float32), z["c"][case.src].astype(np.int32), z["l"][case.src].astype(np.int32), vert, z["scenes"][case.scene].astype(np.float32)


# ------------------------------------------------------------------------------------------------ the Gaussian's pool and cases
GAUSS_DIMS = (6, 8, 10, 12, 14, 16)
GAUSS_PER_DIM = 24
_gauss_pool = None


def gauss_pool():
    """The first GAUSS_PER_DIM inputs of tests/h2_refs.py gauss_eigh_inputs for every dim (all four kinds: well and ill conditioned, rank deficient, below
    the early-out norm), float32: dict(dim[P], grad [P, 16], hess [P, 256] at stride dim, offset [P, 16], H / g / o: the float64 originals per dim)"""
    global _gauss_pool
    if _gauss_pool is None:
        P = GAUSS_PER_DIM * len(GAUSS_DIMS)
        pool = dict(dim=np.zeros(P, np.int32), grad=np.zeros((P, 16), np.float32), hess=np.zeros((P, 256), np.float32), offset=np.zeros((P, 16), np.float32), f64={})
        for k, d in enumerate(GAUSS_DIMS):
            H, g, o = (a[:GAUSS_PER_DIM] for a in h2_refs.gauss_eigh_inputs(d, 512, SIGMA))
            rows = slice(k * GAUSS_PER_DIM, (k + 1) * GAUSS_PER_DIM)
            pool["dim"][rows], pool["grad"][rows, :d], pool["offset"][rows, :d] = d, g, o
            pool["hess"][rows, : d * d] = H.reshape(GAUSS_PER_DIM, d * d)
            pool["f64"][d] = (H, g, o)
        _gauss_pool = pool
    return _gauss_pool


def gauss_states_of_dim(d):
    return np.flatnonzero(gauss_pool()["dim"] == d)


def gauss_techs():
    """every technique of dim 6 to 16 (c + l from 4 to 9)"""
    return [t for t in range(NTECH) if tech_dim(t) >= 6]


def golden_techs():
    z = golden()
    return sorted(set(int(t) for t in z["tech"]))


def _gauss_case(name, pops, seed, stage, grid_blocks):
    pool = gauss_pool()
    src, items, count, start = _lay_out(pops, lambda b: gauss_states_of_dim(tech_dim(b // NSIG)), np.arange(len(pool["dim"])), seed)
    rng = np.random.default_rng(seed + 1)
    flags = (rng.integers(0, 1024, len(src)) & ~F_GSEL) | np.where(rng.random(len(src)) < 0.5, F_GSEL, 0)  # the launch reads F_GSEL alone
    return Case(name, "h2_gauss", src, items, count, start, grid_blocks, flags=flags.astype(np.int32), stage=stage, sigma=SIGMA)


def gauss_count_edge_case(kind, stage=1):
    k = POPULATION_KINDS.index(kind)
    pops = {t * NSIG + (t + k) % NSIG: population(kind, 4) for t in golden_techs()}
    return _gauss_case("count/h2_gauss/%s" % kind, pops, 500 + k, stage, 1024)


def gauss_mixed_case(stage, grid_blocks=1024):
    """dims 6 to 16 in one launch: every technique of those dims over all its eight bins, F_GSEL on about half the chains"""
    return _gauss_case("mixed/h2_gauss/stage%d" % stage, _mixed_pops("h2_gauss", gauss_techs()), 900, stage, grid_blocks)


def gauss_inputs(case, pool=None):
    """the arrays lmc_h2_gauss_list_probe takes: dim[N], grad [N, 16], hess [N, 256], flags[N], offset [N, 16]"""
    pool = pool or gauss_pool()
    return pool["dim"][case.src], pool["grad"][case.src], pool["hess"][case.src], case.flags, pool["offset"][case.src]


GAUSS_NONFINITE_DIM = 8
EARLYOUT_NORM = 0.5 / (SIGMA * SIGMA)


def gauss_nonfinite_case(where, group):
    """One task of four states of dim 8, all far above the early-out norm (dense records); a copy of the pool with state `group` of the task made
    non-finite: where = "hess": +inf in an entry of the triangle the launch reads; "grad": NaN in a gradient entry.  Returns (case, pool, bad chain)."""
    d = GAUSS_NONFINITE_DIM
    base = gauss_pool()
    norms = np.sqrt((base["hess"].astype(np.float64) ** 2).sum(axis=1))
    four = [i for i in gauss_states_of_dim(d) if norms[i] > 4 * EARLYOUT_NORM][:4]
    assert len(four) == 4
    pool = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
    bad = four[group]
    if where == "hess":
        pool["hess"][bad, 1 * d + 3] = np.inf  # row 1, column 3: above the diagonal
    else:
        pool["grad"][bad, 2] = np.nan
    t = tech_index(d // 2 + 1 - 2, 2)  # a technique of that dim with a light sub-path
    count, start = np.zeros(BINS, np.int32), np.zeros(BINS, np.int32)
    count[t * NSIG + 5] = 4
    case = Case("nonfinite/%s/group%d" % (where, group), "h2_gauss", four, np.arange(4), count, start, 2, flags=np.zeros(4, np.int32), stage=1, sigma=SIGMA)
    return case, pool, group


# ------------------------------------------------------------------------------------------------ the walk of the task list, as documented
WALK_MISTAKES = ("no_start", "count_not_reduced", "bin_from_w")


def model_walk(case, mistake=None):
    """dh2coop.h in plain Python: the bins' task counts, their inclusive prefix, and for every task w of the grid-stride loop the reversed index
    wr = total - 1 - w, its bin (the first whose prefix exceeds wr), its number j within the bin and the positions [first, first + n) of `items` it takes.
    Returns [(chain, technique the task runs it as)], chain None where a position lies outside `items` (a device would read whatever is there and use it
    as a chain index).  The grid only distributes the tasks, so it does not appear.  mistake: one of WALK_MISTAKES -- start[bin] dropped, n = min(ipw, count)
    instead of min(ipw, count - first), the bin looked up with w instead of wr.  The last two index outside `items` on almost any list, which is why they are
    shown here and not by running a broken kernel on a device."""
    per = [ipw(case.kernel, b // NSIG) for b in range(BINS)]
    incl = np.cumsum([(int(case.count[b]) + per[b] - 1) // per[b] for b in range(BINS)])
    total, out = int(incl[-1]), []
    for w in range(total):
        wr = total - 1 - w
        b = int(np.searchsorted(incl, w if mistake == "bin_from_w" else wr, side="right"))
        j = wr - (int(incl[b - 1]) if b else 0)
        first = j * per[b]
        n = min(per[b], int(case.count[b]) - (0 if mistake == "count_not_reduced" else first))
        at = (0 if mistake == "no_start" else int(case.start[b])) + first
        out += [(int(case.items[p]) if 0 <= p < case.n_list else None, b // NSIG) for p in range(at, at + n)]
    return out


# ------------------------------------------------------------------------------------------------ the probes' validity rules, restated
def check_valid(N, n_list, items, count, start, grid_blocks, fits):
    """The rules of include/lmc_abi.h for a work list (fits(chain, technique): the chain's state is one of that technique -- of its dim, for the Gaussian);
    returns None or the name of the argument a probe would refuse"""
    if n_list < 1:
        return "n_list"
    if N < n_list:
        return "N"
    if not 1 <= grid_blocks <= GRID_MAX:
        return "grid_blocks"
    items = np.asarray(items)
    if ((items < 0) | (items >= N)).any() or len(np.unique(items)) != len(items):
        return "items"
    if (np.asarray(count) < 0).any():
        return "count"
    used = np.zeros(n_list, int)
    for b in range(BINS):
        if count[b] == 0:
            continue
        if start[b] < 0 or start[b] + count[b] > n_list:
            return "start"
        used[start[b]: start[b] + count[b]] += 1
        if not all(fits(int(i), b // NSIG) for i in items[start[b]: start[b] + count[b]]):
            return "technique"
    return "start" if (used > 1).any() else None


def case_problem(case):
    if case.kernel == "h2_gauss":
        dims = gauss_pool()["dim"][case.src]
        fits = lambda i, t: tech_dim(t) == dims[i]
    else:
        tech = golden()["tech"][case.src]
        fits = lambda i, t: tech[i] == t
    return check_valid(case.N, case.n_list, case.items, case.count, case.start, case.grid_blocks, fits)
