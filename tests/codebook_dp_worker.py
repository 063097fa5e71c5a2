"""One data-parallel rank of tests/test_codebook_gpu.py::test_two_ranks_apply_the_same_update (started as a FRESH process,
never imported by pytest).

    RANK=r WORLD_SIZE=2 MASTER_ADDR=127.0.0.1 MASTER_PORT=p python tests/codebook_dp_worker.py <out_dir> <codebook_restart>

dp_worker.py's tiny model and shared 4-row batch, codebook_ema 0.9: two model.train_step calls on this rank's shard with
parallel.GradAllReduce attached (gloo: the ranks share one GPU), then the codebook, its moving averages and what step 1 left
(this rank's z_e, the summed counts, the embedding, the update's info) are written to <out_dir>/rank<r>.pt."""
import importlib
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))


def main():
    out_dir, tau = sys.argv[1], float(sys.argv[2])
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    pkg = importlib.import_module('vq-vae-wavenet_amd')
    import dp_worker
    torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', '0')) % torch.cuda.device_count())
    dist.init_process_group('gloo', rank=rank, world_size=world)
    m, w, P, x, spk = dp_worker.shared_problem()
    model = pkg.model.VQVAE(dict(m, codebook_ema=0.9, codebook_restart=tau), w, 10, device='cuda', seed=0)
    model.load_named(P)
    model.grad_sync = pkg.parallel.GradAllReduce(model.grad)
    per = x.shape[0] // world
    rows = slice(rank * per, (rank + 1) * per)
    xd, sd = x[rows].contiguous().cuda(), spk[rows].contiguous().cuda()
    ws = model.train_step(xd, sd)
    torch.cuda.synchronize()
    out = {'z_e_1': ws['z_e'].cpu(), 'cnt_1': ws['cb_cnt'].cpu(), 'embedding_1': model.P['embedding'].cpu(),
           'info_1': torch.tensor([model.codebook_info()[k] for k in ('restarted', 'used')]),
           'frames': torch.tensor(ws['B'] * ws['Tz'])}
    model.train_step(xd.flip(0).contiguous(), sd.flip(0).contiguous())
    torch.cuda.synchronize()
    out.update(embedding=model.P['embedding'].cpu(), vq_ema_n=model.vq_ema_n.cpu(), vq_ema_m=model.vq_ema_m.cpu())
    torch.save(out, os.path.join(out_dir, 'rank%d.pt' % rank))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
