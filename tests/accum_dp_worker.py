"""One data-parallel rank of tests/test_accum_gpu.py::test_two_ranks_exchange_once_per_window (started as a FRESH process, never
run by pytest itself; the test imports problem() alone).

    RANK=r WORLD_SIZE=2 MASTER_ADDR=127.0.0.1 MASTER_PORT=p python tests/accum_dp_worker.py <out_dir> gloo

dp_worker.shared_problem's tiny model and weights over eight rows: micro-batch j is rows 2j, 2j + 1; rank r takes micro-batches
2r and 2r + 1 as ONE window of accumulate = 2 with parallel.GradAllReduce attached.  dist.all_reduce is wrapped (as dp_worker's
rccl_one_rank does) to count the SUM calls of the window; the same count is then taken over one normal step (accumulate = 1) of
the same model.  Several ranks share one GPU here, so the backend is gloo.
"""
import importlib
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))


def problem():
    import dp_worker
    from oracle import ref_model as M
    m, w, P, _, _ = dp_worker.shared_problem()
    x, spk, _ = M.synthetic_batch(8, 512, 10, 9)
    return m, w, P, x[:, :, 0].contiguous(), spk


def main():
    out_dir, backend = sys.argv[1], sys.argv[2]
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    pkg = importlib.import_module('vq-vae-wavenet_amd')
    torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', '0')) % torch.cuda.device_count())
    dist.init_process_group(backend, rank=rank, world_size=world)
    m, w, P, x, spk = problem()
    model = pkg.model.VQVAE(m, w, 10, device='cuda', seed=0)
    model.load_named(P)
    model.grad_sync = pkg.parallel.GradAllReduce(model.grad)
    seen = {'sum': 0}
    real_all_reduce = dist.all_reduce

    def counted_all_reduce(t, op=dist.ReduceOp.SUM, group=None, async_op=False):
        if op == dist.ReduceOp.SUM:
            seen['sum'] += 1
        return real_all_reduce(t, op=op, group=group, async_op=async_op)
    dist.all_reduce = counted_all_reduce
    try:
        model.accumulate = 2
        for j in (2 * rank, 2 * rank + 1):
            rows = slice(2 * j, 2 * j + 2)
            model.train_step(x[rows].contiguous().cuda(), spk[rows].contiguous().cuda())
        model.finish_steps()
        torch.cuda.synchronize()
        window_calls, seen['sum'] = seen['sum'], 0
        result = {'grad': model.grad.cpu(), 'flat': model.flat.cpu(), 'ema': model.ema.cpu(),
                  'global_step': torch.tensor(model.global_step), 'accum_index': torch.tensor(model.accum_index)}
        model.accumulate = 1               # one normal step, for its number of exchanges
        rows = slice(2 * rank, 2 * rank + 2)
        model.train_step(x[rows].contiguous().cuda(), spk[rows].contiguous().cuda())
        model.finish_steps()
        torch.cuda.synchronize()
    finally:
        dist.all_reduce = real_all_reduce
    result.update(sum_calls_window=torch.tensor(window_calls), sum_calls_normal=torch.tensor(seen['sum']))
    torch.save(result, os.path.join(out_dir, 'rank%d.pt' % rank))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
