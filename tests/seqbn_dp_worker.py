"""Worker of tests/test_gpu_seqbn.py, one process per GPU under torch.distributed.run: the running
moments of GRU(batch_norm=True) in a data-parallel step.  Every rank trains one step on ITS shard
(unequal lengths, uneven shards); the moments blocks (about the common running mean, weight |V|
of the shard) ride behind the gradients through the step's all-reduce, and every rank applies
the same EMA of the UNION batch's valid-frame moments.  Prints ONE line ``RESULT {json}`` on
rank 0.  Runs at W = 1 too (ASR_FORCE_ALLREDUCE=1: the collective is an identity)."""
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from asr_study_amd import parallel
    from asr_study_amd.core import models, optimizers
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    torch.cuda.set_device(local)
    dev = torch.device('cuda', local)
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29577')
    dist.init_process_group('nccl', rank=rank, world_size=world, device_id=dev)
    rs = np.random.RandomState(0)                       # the same global batch on every rank
    F, C, T = 16, 7, 37
    n_global = 4 * world + 3
    x = (rs.randn(n_global, T, F) * 2 + 1).astype(np.float32)
    lens = rs.randint(5, T + 1, size=n_global)
    lens[0] = T
    for n in range(n_global):
        x[n, lens[n]:] = 0
    labels = [rs.randint(0, C - 1, size=2).tolist() for _ in range(n_global)]
    model = models.deep_speech2(num_features=F, num_classes=C, num_hiddens=18, num_layers=2,
                                conv_filters=4, conv_kernels=((5, 7), (3, 5)), seed=1,
                                dropout=0.0, rnn_type='gru', batch_norm='recurrent', device=dev)
    model.compile(optimizer=optimizers.Adam(lr=1e-3, clipnorm=400))
    w = model.get_weights()
    rw = np.random.RandomState(1)
    for i, a in enumerate(w):                           # running moments away from 0 / 1
        if a.shape == (54,) and i % 6 in (4, 5) and i >= 12:
            w[i] = (rw.rand(54) + 0.5).astype(np.float32) if np.all(a == 1) \
                else (rw.randn(54) * 0.3).astype(np.float32)
    model.set_weights(w)
    parallel.broadcast_parameters(model)
    gru = [(si, s) for si, s in enumerate(model.stages) if s.kind == 'bigru']
    run0 = model.bn_running.cpu().numpy().astype(np.float64)
    keep = parallel.shard_indices(np.arange(n_global), rank, world)
    slab = model.to_slab(x[keep])
    model.train_on_batch(parallel.ShardedBatch([('slab', slab), [labels[i] for i in keep],
                                                lens[keep]], n_global, len(keep)))
    torch.cuda.synchronize()
    mine = {'lens': model._acts[gru[0][0]]['lens'].cpu().numpy()[:len(keep)],
            'p': [model._acts[si]['p'][:, :len(keep)].cpu().numpy().astype(np.float64)
                  for si, _ in gru],
            'run': model.bn_running.cpu().numpy()}
    every = [None] * world
    dist.all_gather_object(every, mine)
    out = {'world': world, 'stages': len(gru)}
    if rank == 0:
        Tr = every[0]['p'][0].shape[0]
        V = np.concatenate([np.arange(Tr)[:, None] < e['lens'][None, :] for e in every], axis=1)
        out['valid_frames_all_ranks'] = int(V.sum())
        out['w_pooled'] = int(round(float(
            model._gbuf[model.n_params + gru[0][1].omom].item())))
        run = every[0]['run'].astype(np.float64)
        em = ev = 0.0
        for k, (si, s) in enumerate(gru):
            Wd = 6 * s.Hp
            rows = np.concatenate([e['p'][k] for e in every], axis=1)[V]
            real = np.tile(np.arange(s.Hp) < s.H, 6)
            for off, batch in ((0, rows.mean(axis=0)), (Wd, rows.var(axis=0))):
                r0 = run0[s.orun + off:s.orun + off + Wd]
                want = s.bn_momentum * r0 + (1.0 - s.bn_momentum) * batch
                err = np.abs(run[s.orun + off:s.orun + off + Wd] - want)[real].max() \
                    / np.abs(want[real]).max()
                if off:
                    ev = max(ev, float(err))
                else:
                    em = max(em, float(err))
        out['running_mean_err'], out['running_var_err'] = em, ev
        out['ranks_agree'] = all(np.array_equal(e['run'], every[0]['run']) for e in every)
        print('RESULT ' + json.dumps(out))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
