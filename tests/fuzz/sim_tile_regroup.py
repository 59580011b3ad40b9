"""Test-infrastructure study (drives the oracle): forming admm_tile16.hip's tiles from instances that share a reference window
(tiny_batch_set_tile_grouping).

The sixteen instances of a wave run in lock step until the slowest has converged: a tile costs the LARGEST of its sixteen iteration counts,
1.125 x their mean when tiles are sixteen consecutive instances of a tracking batch.  The count follows the window start (correlation 0.82 on the
bench batch, standard deviation 1.4 inside one start against 2.9 overall) and nothing a predictor sees explains the rest, so the library sorts
the instances by window start (a counting sort; the order inside one start is free) and cuts the sorted list into tiles.  This script replays
the oracle's TRUE iteration counts as tests/fuzz/sim_tile_deque.py does — 1 024 one-wave-per-SIMD slots, 3.5 iterations of fixed cost per tile,
tiles queued longest first by the predictor's key (exact, and bucketed as dispatch_order.hip's 2 048-bucket sort leaves it), every k-th slot
claiming from the short end — for tiles in index order and tiles by window start, and for a batch whose instance order is shuffled (index-order
tiles then mix every start: the case a caller is most likely to have).  DESIGN.md 5.4 quotes its output.

    python tests/fuzz/sim_tile_regroup.py [batch,seed[,shuffle] ...]

group_by_start / tile_counts / lock_step are imported by tests/test_tile_grouping*.py."""
import sys, heapq, numpy as np

FIX, SLOTS = 3.5, 1024
BENCH = (65536, 20241024)   # bench.py's batch: problems.tracking_batch's default seed
CASES = [BENCH + (0,), (65536, 7, 0), (49152, 4, 0), (98304, 5, 0), (40960, 3, 0), BENCH + (1,)]


def group_by_start(start):
    """The instance map: the instances sorted by window start (stable here; the library's order inside one start is arbitrary), then -1 for the
    padding columns of the last tile.  int32 [16 ceil(B / 16)]."""
    start = np.asarray(start)
    B = len(start)
    m = np.full((B + 15) // 16 * 16, -1, np.int32)
    m[:B] = np.argsort(start, kind="stable")
    return m


def identity_map(B):
    m = np.full((B + 15) // 16 * 16, -1, np.int32)
    m[:B] = np.arange(B)
    return m


def tile_counts(it, imap):
    """lock-step iteration count of every tile: the largest count of the instances its sixteen columns serve (padding columns count nothing)"""
    it = np.asarray(it, np.int64)
    cols = np.where(imap >= 0, it[np.maximum(imap, 0)], 0).reshape(-1, 16)
    return cols.max(1)


def lock_step(it, imap):
    """mean over tiles of the largest count / mean count of the instances"""
    return float(tile_counts(it, imap).mean() / np.asarray(it, np.float64).mean())


def tile_keys(key, imap):
    return np.where(imap >= 0, key[np.maximum(imap, 0)], 0.0).reshape(-1, 16).max(1)


def bucket(key):
    """dispatch_order.hip: sign-less float bits >> 20 (exponent and three mantissa bits), 2 048 buckets"""
    return ((np.asarray(key, np.float32).view(np.uint32) & 0x7fffffff) >> 20).astype(np.int64)


def makespan(tiles_in_order, stride):
    """tiles_in_order: lock-step iteration counts in queue order (predicted longest first); every stride-th slot claims from the short end"""
    n, h, t, mk = len(tiles_in_order), 0, 0, 0.0
    slots = [(0.0, s) for s in range(SLOTS)]; heapq.heapify(slots)
    while h + t < n:
        e, s = heapq.heappop(slots)
        if stride and s % stride == 0: j = n - 1 - t; t += 1
        else: j = h; h += 1
        e += FIX + tiles_in_order[j]; mk = max(mk, e); heapq.heappush(slots, (e, s))
    return mk


def workload(B, seed, shuffle=False, nthreads=8):
    """(true iteration counts, predictor key, window starts) of a tracking batch; shuffle: the instances in a random order"""
    sys.path.insert(0, str(__import__('pathlib').Path(__file__).resolve().parents[2]))
    import accelerated_tinympc_amd as T
    from oracle import oracle as O
    pr = T.problems
    N = 30
    prob = pr.quadrotor(20, N)
    xmn, xmx, umn, umx = pr.bounds_arrays(prob)
    A, Bm, K = (prob[k].astype(np.float64) for k in ("Adyn", "Bdyn", "Kinf"))
    x0, table, start = pr.tracking_batch(B, N, seed=seed)
    if shuffle:
        perm = np.random.default_rng(seed + 1).permutation(B)
        x0, start = x0[perm], start[perm]
    st = O.new_state(B, 12, 4, N); st["x"][:, 0] = x0
    O.Oracle(prob, np.float32, dict(O.DEFAULT_SETTINGS, max_iter=100)).solve(st, xmn, xmx, umn, umx, pr.expand_windows(table, start, N), nthreads=nthreads)
    x = x0.astype(np.float64); key = np.zeros(B)
    for i in range(4):  # dispatch_order.hip's predictor: largest primal residual of the LQR rollout over four steps
        u = -(x @ K.T)
        key = np.maximum(key, np.max(np.abs(x - np.clip(x, -5, 5)), axis=1)); key = np.maximum(key, np.max(np.abs(u - np.clip(u, -0.5, 0.5)), axis=1))
        x = x @ A.T + u @ Bm.T
    return st["iter"].astype(np.int64), key, start


def report(B, seed, shuffle):
    it, key, start = workload(B, seed, bool(shuffle))
    for name, imap in (("index order", identity_map(B)), ("by window start", group_by_start(start))):
        tiles, tk = tile_counts(it, imap), tile_keys(key, imap)
        out = []
        for kname, k in (("bucketed", bucket(tk).astype(np.float64)), ("exact", tk)):
            q = tiles[np.argsort(-k, kind="stable")]
            out.append(f"{kname} key " + " / ".join(f"{makespan(q, s):6.1f}" for s in (0, 4, 8)))
        print(f"B={B:6d} seed {seed}{' shuffled' if shuffle else '':9s} {name:16s} lock step {lock_step(it, imap):.3f}  work per slot {(tiles.sum() + FIX * len(tiles)) / SLOTS:6.1f}  "
              f"makespan at stride 0 / 4 / 8: " + "   ".join(out), flush=True)


if __name__ == "__main__":
    cases = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:]] or CASES
    for c in cases:
        report(c[0], c[1], c[2] if len(c) > 2 else 0)
