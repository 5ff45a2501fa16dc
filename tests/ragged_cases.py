"""The ragged multi-hot requests of the ragged-bucket tests (test_graph_ragged_host.py checks them on the CPU, test_gpu_graph_ragged.py
runs them): host tensors, made from a seed or from explicit bag lengths, and the ORACLE's batch — the standard padded batch whose eager
forward a ragged bucket must reproduce on rows < n: X padded with zero rows, offsets cat(off_req, full(bucket - n, nnz_k)), the ids as they
are."""
import torch

ROWS = [50, 120, 200]
T = len(ROWS)
M_DEN = 4
BATCH_SIZES = (8, 32)
CAPACITY = 3                    # Lcap = 24 / 96


def make_request(n, seed, lens=None, max_len=3, idt=torch.int64, same_nnz=False):
    """-> X [n, M_DEN], offsets (T tensors of n), ids (T tensors of nnz_k), all on the host.  lens: T sequences of n bag lengths; else every
    bag draws its own length in 0 .. max_len (same_nnz: table k's lengths are table 0's rotated by k — what a stacked request needs)"""
    g = torch.Generator().manual_seed(seed)
    X = torch.rand((n, M_DEN), generator=g)
    if lens is None:
        lens = [torch.randint(0, max_len + 1, (n,), generator=g) for _ in ROWS]
        if same_nnz:
            lens = [torch.roll(lens[0], k) for k in range(T)]
    lens = [torch.as_tensor(l, dtype=torch.int64) for l in lens]
    assert len(lens) == T and all(l.numel() == n for l in lens)
    offs = [(torch.cumsum(l, 0) - l).to(idt) for l in lens]
    ids = [torch.randint(0, r, (int(l.sum()),), generator=g, dtype=torch.int64).to(idt) for r, l in zip(ROWS, lens)]
    return X, offs, ids


def padded(bucket, X, offs, ids):
    """the oracle's batch of a request in a bucket"""
    n = X.size(0)
    Xp = torch.zeros((bucket, X.size(1)), dtype=X.dtype)
    Xp[:n] = X
    offs_p = [torch.cat([o, torch.full((bucket - n,), i.numel(), dtype=o.dtype)]) for o, i in zip(offs, ids)]
    return Xp, offs_p, [i.clone() for i in ids]


def well_formed(offs, ids, bags):
    """every table: `bags` offsets that start at 0, never decrease and end inside the ids; every id a row of its table"""
    for o, i, r in zip(offs, ids, ROWS):
        if o.numel() != bags or int(o[0]) != 0 or bool((o[1:] < o[:-1]).any()) or int(o[-1]) > i.numel():
            return False
        if i.numel() and (int(i.min()) < 0 or int(i.max()) >= r):
            return False
    return True


# (name, n, bag lengths per table): the edge cases, all in the bucket of 8 with Lcap = 24
EDGE_CASES = [
    ("empty bags at the head, in the middle and at the end", 6, [[0, 2, 0, 0, 3, 0], [0, 0, 1, 2, 0, 1], [1, 0, 3, 0, 0, 0]]),
    ("n == bucket with a non-empty last bag", 8, [[1, 0, 2, 1, 3, 0, 1, 3], [2, 2, 0, 1, 1, 1, 0, 2], [0, 1, 1, 1, 3, 3, 2, 1]]),
    ("nnz == Lcap for table 0: shift 0", 8, [[3] * 8, [1, 2, 3, 0, 1, 2, 3, 0], [3, 3, 3, 3, 3, 3, 3, 2]]),
    ("one table without a lookup", 5, [[1, 2, 0, 3, 1], [0] * 5, [2, 0, 0, 1, 3]]),
    ("one row", 1, [[2], [0], [3]]),
    ("every bag of its own length", 7, [[3, 1, 2, 0, 1, 3, 2], [1, 1, 2, 2, 3, 3, 0], [0, 3, 0, 3, 0, 3, 1]]),
]
