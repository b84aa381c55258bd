"""The reference's training loop (codes/train.py with model VideoSR_base, ``which_model_G: LIIF``) on the engine.

  python tools/train.py --opt train.yml [--deterministic] [--bench-data N]
  python -m torch.distributed.run --nproc-per-node=8 tools/train.py --opt train.yml [--backend nccl|gloo] [--device K]

The option file is the reference's (options/train/train_zsm.yml), read with serving.parse_options(is_train=True).
Keys used:
  datasets.train   dataroot_GT (the folder of frame folders), video_list (a text file, one folder name per line;
                   default: every sub-folder of dataroot_GT), batch_size, n_workers, lq_size (default 64: the
                   reference's collate constant; the LQ side is lq_size / 2)
  network_G        which_model_G (LIIF), front_RBs, back_RBs
  path             pretrain_model_G + strict_load, resume_state, models, training_state
  train            lr_G, beta1, beta2, weight_decay_G, lr_scheme and its keys (train.make_optimizer), niter,
                   warmup_iter, pixel_criterion (cb), pixel_weight, manual_seed
  logger           print_freq, save_checkpoint_freq

Per iteration (train.py:165-178, VideoSR_base_model.py:113-134): update_learning_rate, then optimize_step on
``net(LQs, time, shape)`` with TimesLoss(CharbonnierLoss()) * pixel_weight.  Batches come from data.BatchLoader:
batch i is a pure function of (manual_seed, i) and iteration k trains on batch k - 1, so ``path.resume_state`` needs no
sampler state.  The f16x3 range status is read every print_freq iterations only (the read is one synchronisation)
and logged when it is not zero.  Every save_checkpoint_freq iterations: ``{iter}_G.pth`` under path.models (the CPU
state dict, the reference's 442 keys) and ``{iter}.state`` under path.training_state (the reference's epoch / iter /
schedulers / optimizers, plus seed).  Resuming loads ``{iter}_G.pth`` beside the state, as options.check_resume does.

Under torch.distributed.run (RANK / WORLD_SIZE / LOCAL_RANK in the environment) the loop is data-parallel (DESIGN.md
section 3r): ``init_process_group(--backend)``, one rank per card (``cuda:LOCAL_RANK``; ``--device K`` pins every rank
to card K, which with ``--backend gloo`` lets ranks share a GPU), ``datasets.train.batch_size`` stays the global batch
and rank r trains on its ``data.rank_items`` through ``train.DataParallel``: gradients are summed over the ranks -- not
averaged, the loss is a sum -- in rank order under ``--deterministic``.  Every rank loads the same pretrain / resume
files; rank 0 alone logs and writes the checkpoints, in the same formats, so a checkpoint resumes on any number of
ranks.  The logged l_pix is the sum over the ranks, and it and the range status (ORed over the ranks) are read at
print_freq only.  At each save the ranks compare a checksum of their parameters and the run aborts if the replicas
diverged.  Worker threads per rank: n_workers, capped so that ranks x workers <= 16.  Started plainly, the script is
the single-process loop it was.

Not built: overlap of the gradient exchange with the backward, multi-node runs, validation during training (val_freq),
the tensorboard logger, and the l1 / l2 / lp criteria (NotImplementedError names the key).

--bench-data N: iterations per second over N iterations with the loader, and over N iterations on one pre-built
batch; the gap is what the data path costs inside training.
"""
import argparse
import json
import math
import os
import random
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stif_pkg  # noqa: E402


RANK, WORLD = 0, 1     # set by main() under torch.distributed.run


def log(msg):
    if RANK == 0:
        print(msg, flush=True)


def make_loader(stif, opt, seed, start=0, device="cuda"):
    ds = opt["datasets"]["train"]
    root = os.path.expanduser(ds["dataroot_GT"])
    if ds.get("video_list"):
        with open(os.path.expanduser(ds["video_list"])) as f:
            videos = [v.strip() for v in f if v.strip()]
    else:
        videos = sorted(d for d in os.listdir(root) if os.path.isdir(os.path.join(root, d)))
    index = stif.data.ClipIndex(root, videos)
    log(f"dataset: {len(videos)} videos, {len(index)} windows under {root}")
    workers = ds.get("n_workers", 4)
    if WORLD > 1:
        return stif.data.BatchLoader(index, ds["batch_size"], seed, lq_size=ds.get("lq_size", 64),
                                     workers=min(workers, 16 // WORLD), device=device, start=start, rank=RANK,
                                     world=WORLD)
    return stif.data.BatchLoader(index, ds["batch_size"], seed, lq_size=ds.get("lq_size", 64),
                                 workers=workers, device=device, start=start)


def make_criterion(TR, train_opt):
    kind = train_opt.get("pixel_criterion", "cb")
    if kind == "cb":
        return TR.TimesLoss(TR.CharbonnierLoss())
    if kind in ("l1", "l2", "lp"):
        raise NotImplementedError(f"train.pixel_criterion: {kind!r} is not built (cb only)")
    raise NotImplementedError(f"train.pixel_criterion: {kind!r} is not recognized")


def save(net, optimizer, scheduler, opt, it, epoch, seed):
    for key in ("models", "training_state"):
        os.makedirs(opt["path"][key], exist_ok=True)
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    torch.save(sd, os.path.join(opt["path"]["models"], f"{it}_G.pth"))
    state = {"epoch": epoch, "iter": it, "schedulers": [scheduler.state_dict()],
             "optimizers": [optimizer.state_dict()], "seed": seed}
    torch.save(state, os.path.join(opt["path"]["training_state"], f"{it}.state"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--opt", required=True)
    ap.add_argument("--deterministic", action="store_true", help="train.set_deterministic(True)")
    ap.add_argument("--bench-data", type=int, default=0, metavar="N")
    ap.add_argument("--backend", choices=("nccl", "gloo"), default="nccl", help="under torch.distributed.run")
    ap.add_argument("--device", type=int, default=None, metavar="K",
                    help="under torch.distributed.run: every rank on cuda:K instead of cuda:LOCAL_RANK")
    args = ap.parse_args()
    distributed = "RANK" in os.environ and "WORLD_SIZE" in os.environ
    if distributed and args.bench_data:
        ap.error("--bench-data is a single-process measurement")
    stif = stif_pkg.load()
    TR, S = stif.train, stif.serving
    opt = S.parse_options(args.opt, is_train=True)
    train_opt, net_opt, paths = opt["train"], opt["network_G"], opt.get("path") or {}
    if net_opt["which_model_G"] != "LIIF":
        raise NotImplementedError(f"network_G.which_model_G: {net_opt['which_model_G']!r} (LIIF only)")
    assert torch.cuda.is_available(), "training needs the GPU"
    dev = torch.device("cuda", 0)
    if distributed:
        import torch.distributed as dist
        global RANK, WORLD
        dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0)) if args.device is None else args.device)
        torch.cuda.set_device(dev)
        dist.init_process_group(args.backend)
        RANK, WORLD = dist.get_rank(), dist.get_world_size()
        log(f"data-parallel: {WORLD} ranks, backend {args.backend}, rank 0 on {dev}")

    resume = None
    if paths.get("resume_state"):
        # the file is this script's own checkpoint: optimizer and schedule state, not only tensors
        resume = torch.load(paths["resume_state"], map_location="cpu", weights_only=False)
    seed = resume["seed"] if resume else train_opt.get("manual_seed")
    if seed is None:
        seed = random.randint(1, 10000)
        if WORLD > 1:      # one draw for all ranks: the batches are a function of the seed
            box = [seed]
            dist.broadcast_object_list(box, src=0)
            seed = box[0]
    log(f"random seed: {seed}")
    random.seed(seed)
    torch.manual_seed(seed)
    TR.set_deterministic(args.deterministic)

    criterion = make_criterion(TR, train_opt)
    net = TR.LunaTokis(net_opt["front_RBs"], net_opt["back_RBs"])
    pretrain, strict = paths.get("pretrain_model_G"), bool(paths.get("strict_load", True))
    if resume:
        pretrain, strict = os.path.join(paths["models"], f"{resume['iter']}_G.pth"), True
    if pretrain:
        log(f"loading model for G [{pretrain}] (strict: {strict})")
        S.load_network(pretrain, net, strict)
    net = net.to(dev)
    optimizer, scheduler = TR.make_optimizer(net, train_opt)
    start = 0
    if resume:
        optimizer.load_state_dict(resume["optimizers"][0])
        scheduler.load_state_dict(resume["schedulers"][0])
        start = int(resume["iter"])
        log(f"resuming training from epoch: {resume['epoch']}, iter: {start}")

    weight = float(train_opt.get("pixel_weight", 1.0))
    niter, warmup = int(train_opt["niter"]), int(train_opt.get("warmup_iter", -1))
    lg = opt.get("logger") or {}
    print_freq, save_freq = int(lg.get("print_freq", 100)), int(lg.get("save_checkpoint_freq", 0) or 0)

    def step(batch, it):
        TR.update_learning_rate([scheduler], [optimizer], it, warmup)
        return TR.optimize_step(net, optimizer, criterion, (batch["LQs"], batch["time"], batch["shape"]), batch["GT"],
                                weight)

    if args.bench_data:
        bench_data(stif, opt, seed, step, args.bench_data, dev)
        return

    loader = make_loader(stif, opt, seed, start, dev)
    if distributed:
        try:
            train_ranks(TR, net, optimizer, scheduler, criterion, loader, opt, seed, start, weight, dev)
        finally:
            dist.destroy_process_group()
        return
    batches = iter(loader)
    try:
        for it in range(start + 1, niter + 1):
            loss = step(next(batches), it)
            if not math.isfinite(loss):
                log(f"iter: {it}: l_pix is {loss}")
            if it % print_freq == 0:
                status = TR.range_status(dev)
                lr = optimizer.param_groups[0]["lr"]
                log(f"<epoch:{(it - 1) // loader.per_epoch:3d}, iter:{it:8,d}, lr:({lr:.6e},)> l_pix: {loss:.6e}")
                if status:
                    log(f"iter: {it}: f16x3 range status {status} (an operand left the split-fp16 range since the "
                        f"last report; such steps need mfma=\"f32\")")
            if save_freq and it % save_freq == 0:
                save(net, optimizer, scheduler, opt, it, (it - 1) // loader.per_epoch, seed)
                log(f"saved models and training states at iter {it}")
    finally:
        batches.close()
    log("end of training")


def train_ranks(TR, net, optimizer, scheduler, criterion, loader, opt, seed, start, weight, dev):
    """The loop under torch.distributed.run: DataParallel steps on this rank's items, no host read between print_freq
    iterations, rank 0 logging and saving."""
    train_opt, lg = opt["train"], opt.get("logger") or {}
    niter, warmup = int(train_opt["niter"]), int(train_opt.get("warmup_iter", -1))
    print_freq, save_freq = int(lg.get("print_freq", 100)), int(lg.get("save_checkpoint_freq", 0) or 0)
    dp = TR.DataParallel(net, optimizer)
    batches = iter(loader)
    try:
        for it in range(start + 1, niter + 1):
            batch = next(batches)
            TR.update_learning_rate([scheduler], [optimizer], it, warmup)
            dp.step(criterion, (batch["LQs"], batch["time"], batch["shape"]), batch["GT"], weight)
            if it % print_freq == 0:
                loss, status = dp.global_loss(), dp.range_status()
                lr = optimizer.param_groups[0]["lr"]
                log(f"<epoch:{(it - 1) // loader.per_epoch:3d}, iter:{it:8,d}, lr:({lr:.6e},)> l_pix: {loss:.6e}")
                if status:
                    log(f"iter: {it}: f16x3 range status {status} (an operand left the split-fp16 range on some rank "
                        f"since the last report; such steps need mfma=\"f32\")")
            if save_freq and it % save_freq == 0:
                if not dp.replicas_agree():
                    log(f"iter: {it}: the ranks' parameters differ (checksum mismatch): the replicas diverged; "
                        "aborting without a checkpoint")
                    raise SystemExit(3)
                if RANK == 0:
                    save(net, optimizer, scheduler, opt, it, (it - 1) // loader.per_epoch, seed)
                log(f"saved models and training states at iter {it}")
    finally:
        batches.close()
    log("end of training")


def bench_data(stif, opt, seed, step, n, dev):
    """Iterations per second with the loader against one pre-built batch reused."""
    warm = 2
    loader = make_loader(stif, opt, seed, 0, dev)
    batches = iter(loader)
    try:
        first = next(batches)
        for k in range(warm):
            step(first, k + 1)
        torch.cuda.synchronize()
        res = {}
        t0 = time.perf_counter()
        for k in range(n):
            step(next(batches), warm + k + 1)
        torch.cuda.synchronize()
        res["loader_it_per_s"] = n / (time.perf_counter() - t0)
        t0 = time.perf_counter()
        for k in range(n):
            step(first, warm + n + k + 1)
        torch.cuda.synchronize()
        res["reused_batch_it_per_s"] = n / (time.perf_counter() - t0)
    finally:
        batches.close()
    res.update(iterations=n, batch_size=loader.batch_size, workers=loader.workers, lq_size=loader.lq_size,
               note="the loader's batches vary in GT size with d; the reused batch is batch 0")
    log("bench-data " + json.dumps(res))


if __name__ == "__main__":
    main()
