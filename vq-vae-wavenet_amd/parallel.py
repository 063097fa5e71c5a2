"""Data-parallel gradient exchange: one process per GPU, RCCL (torch.distributed 'nccl') sum
all-reduce of the flat fp32 gradient buffer over xGMI, in buckets that are launched on a side
stream as soon as backward has finished writing them: the decoder gradients (81 MB of 140.6 MB) overlap the
encoder backward, the encoder's 11.8 MB kernels follow layer by layer as their weight gradients finish, so only
the first layers' gradients (12 MB) are exchanged after the last kernel of the step.  The reference has no multi-GPU code
(SURVEY.md 2.1); training shards over batch, all losses are means, BN uses moving statistics,
so averaging the per-rank gradients reproduces the full-batch step.
"""
import torch
import torch.distributed as dist


class GradAllReduce:
    """force=True: run every collective even in a world of one rank (a 1-rank RCCL all-reduce is an identity, but it is the
    real communicator, bucket slices, side-stream joins and flag exchange: how a 1-GPU box exercises the N > 1 code path)."""

    def __init__(self, flat_grad, group=None, force=False):
        self.flat = flat_grad
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0       # (seeds this rank's time-jitter draws)
        self.active = self.world > 1 or (force and dist.is_initialized())
        self.buckets = []           # (lo, hi) of every bucket exchanged since the last finish(), in launch order
        self.cuda = flat_grad.is_cuda
        self.stream = torch.cuda.Stream(device=flat_grad.device) if self.cuda else None
        self.pending = []
        # hold: set by a model that accumulates gradients over micro-batches (WaveNet.accumulate) for every pass of a window --
        # bucket_ready then launches nothing and finish() waits for nothing; the model releases it on the window's last micro-step
        # and hands over the whole flat buffer, the summed gradient, in the ranges the held pass was refused (last_held: the
        # bucket boundaries of a normal step): one exchange per window.  all_reduce_max is never held.
        self.hold = False
        self.held, self.last_held = [], []

    def bucket_ready(self, lo, hi):
        """flat[lo:hi] holds final local gradients: start summing it across ranks."""
        if not self.active or hi <= lo:
            return
        if self.hold:
            self.held.append((lo, hi))
            return
        self.buckets.append((lo, hi))
        view = self.flat[lo:hi]
        if self.cuda:
            self.stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(self.stream):
                dist.all_reduce(view, op=dist.ReduceOp.SUM, group=self.group)
        else:
            self.pending.append(dist.all_reduce(view, op=dist.ReduceOp.SUM, group=self.group, async_op=True))

    def finish(self):
        """Wait for all buckets; returns the world size (the caller scales by 1/world).  Held: nothing was launched, nothing to wait for."""
        if self.hold:
            self.last_held, self.held = self.held, []
            return self.world
        if self.cuda and self.active:
            torch.cuda.current_stream().wait_stream(self.stream)
        for w in self.pending:
            w.wait()
        self.pending = []
        self.last_buckets, self.buckets = self.buckets, []
        return self.world

    def all_reduce_max(self, t):
        """In-place MAX over the ranks (the fp16x3 engine's range flag: every rank must take the same branch)."""
        if self.active:
            dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.group)
        return t

    def all_reduce_sum(self, t):
        """In-place SUM over the ranks on the caller's stream (the codebook's cluster statistics, DESIGN 3.11: every rank must
        apply the same update).  Active under the same condition as all_reduce_max."""
        if self.active:
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
        return t
