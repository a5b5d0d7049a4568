"""Multi-GPU plumbing: pair-index sharding and the gathers of the sparse posteriors.

Two users.  bench.py times phase 1 at the L0 (device pointer) level: cost-sorted deal of the pair jobs
(shard_pairs) and ONE all-gather of a packed slab per step (ShardExchange).  phase1_sharded is the whole
sharded phase 1 of a run: the library's dafs_hip_phase1_sharded (folds by x mod G, pair posteriors and the
matching consistency transform by contiguous pair-index ranges, each followed by a gather), with
torch.distributed supplying the collective (_allgather_into); after it every rank's context holds the
complete stores and the rest of the run (guide tree, progressive phase) is replicated (SURVEY.md 8e:
phase 2 is tree-sequential).

One process per GPU (torch.distributed; backend "nccl" is RCCL over xGMI on ROCm, "gloo" in the CPU
tests).  The N(N-1)/2 pair jobs are independent: they are sorted by cost and dealt round-robin to the
ranks, every rank runs its shard with no communication, and the sparse posteriors are
exchanged with a single all-gather of fixed-stride slabs.  After it every rank can address every
pair's rows (GatheredPairs), which is what guide-tree construction and the consistency transforms
need.  torch is used for device memory and the collective only.
"""
import numpy as np


def shard_pairs(lens, world, rank):
    """Row-major (i<j) pairs sorted by len_i*len_j descending, dealt round-robin.
    Returns (pair_x, pair_y, total_pairs) of this rank, longest first."""
    lens = np.asarray(lens, dtype=np.int64)
    n = len(lens)
    ii, jj = np.triu_indices(n, k=1)
    order = np.argsort(-(lens[ii] * lens[jj]), kind="stable")
    mine = order[rank::world]
    return ii[mine].astype(np.int64), jj[mine].astype(np.int64), len(order)


def pair_id(x, y, n):
    """row-major index of pair x<y among n sequences"""
    return x * n - x * (x + 1) // 2 + (y - x - 1)


def pair_ranges(npairs, world):
    """[(begin, end)] per rank: the contiguous ranges of the row-major pair enumeration that a sharded phase 1 gives its
    ranks (dafs_hip_pair_range)"""
    return [(npairs * r // world, npairs * (r + 1) // world) for r in range(world)]


class GatheredPairs:
    """Every rank's shard after the all-gather; csr(x, y) returns the rows of mp[x][y] for any x != y."""

    def __init__(self, lens, world, meta, rowptr, col, val, strides):
        self.lens = np.asarray(lens, dtype=np.int64)
        self.n = len(self.lens)
        self.world = world
        self.meta, self.rowptr, self.col, self.val = meta, rowptr, col, val
        self.s_pairs, self.s_rp, self.s_pool = strides
        self._where = {}
        self._rp_off = []
        for r in range(world):
            px, py, _ = shard_pairs(self.lens, world, r)
            sizes = self.lens[px] + 1 + self.lens[py] + 1
            self._rp_off.append(np.concatenate([[0], np.cumsum(sizes)]))
            for k, (x, y) in enumerate(zip(px, py)):
                self._where[(int(x), int(y))] = (r, k)

    def _entry(self, x, y):
        r, k = self._where[(x, y)]
        m = self.meta[(r * self.s_pairs + k) * 4:(r * self.s_pairs + k) * 4 + 4]
        nnz = int(m[0])
        sim = np.array([int(m[1])], np.int32).view(np.float32)[0]
        off = int(np.array([int(m[2]), int(m[3])], np.int32).view(np.int64)[0])
        return r, k, nnz, sim, off

    def sim(self, x, y):
        if x == y:
            return np.float32(1.0)
        return self._entry(min(x, y), max(x, y))[3]

    def sim_matrix(self):
        out = np.eye(self.n, dtype=np.float32)
        for (x, y) in self._where:
            out[x, y] = out[y, x] = self.sim(x, y)
        return out

    def csr(self, x, y):
        a, b = min(x, y), max(x, y)
        r, k, nnz, _, off = self._entry(a, b)
        l1, l2 = int(self.lens[a]) + 1, int(self.lens[b]) + 1
        rp0 = r * self.s_rp + int(self._rp_off[r][k])
        e0 = r * self.s_pool + off
        if x < y:
            return self.rowptr[rp0:rp0 + l1], self.col[e0:e0 + nnz], self.val[e0:e0 + nnz]
        return self.rowptr[rp0 + l1:rp0 + l1 + l2], self.col[e0 + nnz:e0 + 2 * nnz], self.val[e0 + nnz:e0 + 2 * nnz]


    def forward_arrays(self):
        """(nnz, rowptr, col, val) of all pairs in row-major order -- the arguments of Context.set_mp, i.e. how a rank
        takes the gathered shards back into its context for the consistency transforms and the progressive phase."""
        nnz, rps, cols, vals = [], [], [], []
        for x in range(self.n):
            for y in range(x + 1, self.n):
                rp, col, val = self.csr(x, y)
                nnz.append(len(col)); rps.append(rp); cols.append(col); vals.append(val)
        return (np.array(nnz, np.uint32), np.concatenate(rps).astype(np.uint32), np.concatenate(cols).astype(np.uint32),
                np.concatenate(vals).astype(np.float32))


class ShardExchange:
    """The one exchange of phase 1 at the L0 level: every rank's {per-pair nnz / sim / pool offset, row pointers,
    entry columns, entry values} travel as ONE packed int32 slab in ONE all-gather (fixed strides agreed once up
    front; a rank whose parts are shorter pads).  Slab of rank r: [4 * s_pairs meta | s_rp row pointers | s_pool
    columns | s_pool values (bits)]."""

    def __init__(self, dist, device, world, n_pairs_local, rp_total_local, pool_cap_local):
        import torch
        self.dist, self.torch, self.world, self.device = dist, torch, world, device
        sizes = torch.tensor([n_pairs_local, rp_total_local, pool_cap_local], dtype=torch.int64, device=device)
        dist.all_reduce(sizes, op=dist.ReduceOp.MAX)
        self.s_pairs, self.s_rp, self.s_pool_cap = [int(v) for v in sizes.tolist()]
        self.n_pairs, self.rp_total = n_pairs_local, rp_total_local
        self.s_pool = 0
        self.send = self.recv = None

    def _layout(self):
        m, r, c = 4 * self.s_pairs, self.s_rp, self.s_pool
        return m, r, c, m + r + 2 * c

    def exchange(self, pair_nnz, sim, pair_off, rowptr, col, val, pool_used):
        """pair_nnz int32[n], sim float32[n], pair_off int64[n], rowptr int32[rp_total], col int32[cap],
        val float32[cap] (all on self.device); pool_used = entries this rank produced (None: as in the previous
        call).  One max-reduce for the payload stride the first time, then the gather itself."""
        torch, dist = self.torch, self.dist
        if pool_used is None and self.s_pool == 0:
            raise ValueError("ShardExchange.exchange: the first call needs pool_used (the payload stride is agreed from it)")
        if pool_used is not None:
            mx = torch.tensor([int(pool_used)], dtype=torch.int64, device=self.device)
            dist.all_reduce(mx, op=dist.ReduceOp.MAX)
            self.s_pool = int(mx.item())
        # pool_used=None: a repeat of an exchange whose sizes are known (same inputs): the stride agreed then is
        # reused and nothing in this call waits for the device
        m, r, c, total = self._layout()
        if self.send is None or self.send.numel() != total:
            self.send = torch.zeros(total, dtype=torch.int32, device=self.device)
            self.recv = torch.empty(self.world * total, dtype=torch.int32, device=self.device)
        meta = self.send[:m].view(self.s_pairs, 4)
        meta[:self.n_pairs, 0] = pair_nnz
        meta[:self.n_pairs, 1] = sim.view(torch.int32)
        meta[:self.n_pairs, 2:4] = pair_off.view(torch.int32).view(self.n_pairs, 2)
        self.send[m:m + self.rp_total] = rowptr[:self.rp_total]
        k = min(c, col.numel())
        self.send[m + r:m + r + k] = col[:k]
        self.send[m + r + c:m + r + c + k] = val[:k].view(torch.int32)
        dist.all_gather_into_tensor(self.recv, self.send)

    def gathered(self, lens):
        m, r, c, total = self._layout()
        rows = self.recv.cpu().numpy().reshape(self.world, total)
        meta = np.ascontiguousarray(rows[:, :m]).reshape(-1)
        rp = np.ascontiguousarray(rows[:, m:m + r]).reshape(-1).view(np.uint32)
        col = np.ascontiguousarray(rows[:, m + r:m + r + c]).reshape(-1).view(np.uint32)
        val = np.ascontiguousarray(rows[:, m + r + c:]).reshape(-1).view(np.float32)
        return GatheredPairs(lens, self.world, meta, rp, col, val, (self.s_pairs, self.s_rp, self.s_pool))


# ---------------------------------------------------------------------------------------------
# sharded phase 1 of a whole run: dafs_hip_phase1_sharded, torch.distributed as its collective
# ---------------------------------------------------------------------------------------------
def _allgather_into(dist, send_t, recv_t):
    """recv_t[r * n:(r + 1) * n] = send_t of rank r (n elements each), landed when this returns: what dafs_allgather_fn
    promises the library, which enqueues its reads of recv on a stream of its own as soon as the callback returns.  nccl
    (RCCL) gathers on the device; gloo, which the tests with several ranks on one GPU use, through host memory."""
    import torch
    if dist.get_backend() == "nccl":
        dist.all_gather_into_tensor(recv_t, send_t)
    else:
        host = torch.empty(recv_t.shape, dtype=recv_t.dtype)
        dist.all_gather_into_tensor(host, send_t.cpu())
        recv_t.copy_(host)
    if recv_t.is_cuda:
        torch.cuda.synchronize(recv_t.device)


class _DeviceBytes:
    """nbytes of device memory at ptr, in the form torch.as_tensor takes without copying (__cuda_array_interface__)"""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "strides": None, "version": 2}


def phase1_sharded(ctx, seqs, dist, device, align_model, th_a, w_pct_a, w_pct_s, fold_th=0.01):
    """Phase 1 of DAFS::run (dafs.cpp:1787-1827) on `world` ranks, one context (one GPU) each: dafs_hip_phase1_sharded,
    with all_gather_into_tensor on the library's device buffers as the collective.  Afterwards ctx is in the state a
    single-GPU phase 1 leaves it in, bit for bit.  `device` (the rank's GPU) is not needed: the buffers are the library's."""
    import torch
    ctx.set_sequences(seqs)
    if len(seqs) < 2:  # no pairs to share (the library refuses them): every rank runs the phase itself, as dafs --devices does
        ctx.fold_posteriors(fold_th)
        ctx.align_posteriors(align_model, th_a, fetch=False)
        ctx.consistency_match(w_pct_a)
        ctx.consistency_bp(w_pct_s)
        return
    world = dist.get_world_size()

    def allgather(send, recv, nbytes):
        _allgather_into(dist, torch.as_tensor(_DeviceBytes(send, nbytes)), torch.as_tensor(_DeviceBytes(recv, world * nbytes)))

    ctx.phase1_sharded(dist.get_rank(), world, align_model, th_a, w_pct_a, w_pct_s, fold_th, allgather)
