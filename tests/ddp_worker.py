"""One rank of the data-parallel GPU tests (tests/test_gpu_ddp.py), started by torch.distributed.run: gloo process
group, every rank on cuda:0 (one GPU box), the HIP engine as compute.

  ddp_worker.py <outdir> <batch>:<reduce> [<batch>:<reduce> ...]      reduce: auto | ordered | sum

For every configuration in turn: the tiny model of ddp_cases.make_net (ranks other than 0 perturb their parameters
first, so the constructor's broadcast shows), train.DataParallel, two steps under train.deterministic() on this rank's
data.rank_items of ddp_cases.global_batch.  Saved to <outdir>/c<config>_r<rank>.pt: parameters and Adam moments, the
global loss of each step, the arena after step 1 with its layout, the ORed range status, the replica checksum's
verdict."""
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    outdir, configs = sys.argv[1], [c.split(":") for c in sys.argv[2:]]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo")
    import ddp_cases as DC
    import stif_pkg
    stif = stif_pkg.load()
    TR = stif.train
    torch.cuda.set_device(0)
    for ci, (batch, reduce) in enumerate(configs):
        batch = int(batch)
        net, opt, crit = DC.make_net(stif)
        if rank:
            with torch.no_grad():
                for p in net.parameters():
                    p.add_(0.01 * rank)
        dp = TR.DataParallel(net, opt, reduce=None if reduce == "auto" else reduce)
        a, b = stif.data.rank_items(batch, world, rank)
        inputs, gt = DC.rows(DC.global_batch(batch), a, b)
        losses, arena1 = [], None
        with TR.deterministic():
            mode = dp._mode()
            for s in range(DC.STEPS):
                mine = dp.step(crit, inputs, gt)
                assert mine.is_cuda and mine.dim() == 0
                losses.append(dp.global_loss())
                if s == 0:
                    arena1 = dp.arena.arena.cpu().clone()
        res = dict(state=DC.state_of(net, opt), losses=losses, arena1=arena1, names=dp.arena.names,
                   offsets=dp.arena.offsets, sizes=dp.arena.sizes, items=(a, b), mode=mode,
                   status=dp.range_status(), agree=dp.replicas_agree())
        torch.save(res, os.path.join(outdir, f"c{ci}_r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
