"""Data-parallel training on the GPU: real ranks (torch.distributed.run, gloo, all on cuda:0,
tests/ddp_worker.py) against ``train.emulate_ranks`` in this process, bit for bit -- parameters, Adam moments and the
global loss of two steps under ``train.deterministic()`` -- for an even split, an uneven split and three ranks; world 1
against ``optimize_step``; the summed gradient against one process on the whole batch (sum semantics); and
tools/train.py end to end on two ranks, resumed as one process.

Model: the smallest the state-dict spec builds (front_RBs = back_RBs = 1, 270 keys of which 262 receive a gradient), LR
frames 8 x 12 decoded to 16 x 24."""
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import ddp_cases as DC

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _launch(world, args, timeout=240):
    """torch.distributed.run with ``world`` local ranks (a child process; the launcher never touches the GPU)."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr=127.0.0.1", f"--master-port={_free_port()}"] + args
    r = subprocess.run(cmd, cwd=REPO, env=dict(os.environ, OMP_NUM_THREADS="4"), capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


_RUNS = {}
TWO_RANKS = ["2:auto", "3:auto"]      # one launch serves the even split, the uneven split and the sum-semantics test


def ranks(tmp_path_factory, world, configs):
    """The saved results [config][rank] of one worker launch; each launch runs once per session."""
    key = (world, tuple(configs))
    if key not in _RUNS:
        d = str(tmp_path_factory.mktemp(f"ddp_w{world}"))
        _launch(world, ["tests/ddp_worker.py", d] + list(configs))
        _RUNS[key] = [[torch.load(os.path.join(d, f"c{c}_r{r}.pt"), weights_only=True) for r in range(world)]
                      for c in range(len(configs))]
    return _RUNS[key]


_EMULATED = {}


def emulated(stif, batch, world):
    """(state, losses, arena after step 1) of train.emulate_ranks for the split of ``batch`` over ``world``."""
    if (batch, world) not in _EMULATED:
        TR = stif.train
        net, opt, crit = DC.make_net(stif)
        full = DC.global_batch(batch)
        per_rank = [DC.rows(full, *stif.data.rank_items(batch, world, r)) for r in range(world)]
        losses, arena1 = [], None
        with TR.deterministic():
            for s in range(DC.STEPS):
                loss = TR.emulate_ranks(net, opt, crit, per_rank)
                assert loss.is_cuda and loss.dtype == torch.float32
                losses.append(float(loss))
                if s == 0:
                    arena1 = opt.emulated_arena.arena.cpu().clone()
        assert TR.range_status() == 0
        _EMULATED[batch, world] = (DC.state_of(net, opt), losses, arena1)
    return _EMULATED[batch, world]


def assert_same_state(a, b, what):
    assert list(a) == list(b), what
    for k in a:
        assert DC.same_bytes(a[k], b[k]), (what, k)


def check_against_emulation(stif, res, batch, world, bitwise_with_emulation=True):
    state, losses, _ = emulated(stif, batch, world)
    assert sum(k.startswith("p/") for k in state) == DC.KEYS
    assert sum(k.endswith("/exp_avg") for k in state) == DC.COVERED       # Adam moments of the covered keys only
    for r, got in enumerate(res):
        assert tuple(got["items"]) == stif.data.rank_items(batch, world, r)
        assert len(got["names"]) == DC.COVERED and got["status"] == 0 and got["agree"] is True
        assert_same_state(got["state"], res[0]["state"], f"rank {r} against rank 0")
        assert got["losses"] == res[0]["losses"] and all(np.isfinite(v) and v > 0 for v in got["losses"])
        for v in got["state"].values():
            assert bool(torch.isfinite(v.float()).all())
        if bitwise_with_emulation:
            assert_same_state(got["state"], state, f"rank {r} against emulate_ranks")
            print(f"world {world} batch {batch}: global losses {got['losses']} (emulated {losses})")
            assert got["losses"] == losses and losses[0] != losses[1]


def test_two_ranks_even_split_equal_the_emulation_bitwise(stif, tmp_path_factory):
    res = ranks(tmp_path_factory, 2, TWO_RANKS)[0]
    assert [r["mode"] for r in res] == ["ordered", "ordered"]             # the default follows the switch
    check_against_emulation(stif, res, 2, 2)


def test_two_ranks_uneven_split_equal_the_emulation_bitwise(stif, tmp_path_factory):
    res = ranks(tmp_path_factory, 2, TWO_RANKS)[1]
    assert [tuple(r["items"]) for r in res] == [(0, 2), (2, 3)]
    check_against_emulation(stif, res, 3, 2)


def test_three_ranks_ordered_equal_the_emulation_and_sum_keeps_replicas_identical(stif, tmp_path_factory):
    ordered, summed = ranks(tmp_path_factory, 3, ["3:ordered", "3:sum"])
    assert [r["mode"] for r in ordered] == ["ordered"] * 3 and [r["mode"] for r in summed] == ["sum"] * 3
    check_against_emulation(stif, ordered, 3, 3)
    check_against_emulation(stif, summed, 3, 3, bitwise_with_emulation=False)


def test_world_one_step_leaves_what_optimize_step_leaves(stif):
    TR = stif.train
    full = DC.global_batch(2)
    inputs, gt = DC.rows(full, 0, 2)
    with TR.deterministic():
        net_a, opt_a, crit = DC.make_net(stif)
        want = [TR.optimize_step(net_a, opt_a, crit, inputs, gt) for _ in range(DC.STEPS)]
        net_b, opt_b, crit = DC.make_net(stif)
        dp = TR.DataParallel(net_b, opt_b)
        got = []
        for _ in range(DC.STEPS):
            loss = dp.step(crit, inputs, gt)
            assert loss.is_cuda and not loss.requires_grad
            got.append(dp.global_loss())
    assert dp.world == 1 and not dp.distributed and len(dp.arena.names) == DC.COVERED
    assert got == want and dp.range_status() == 0 and dp.replicas_agree()
    assert_same_state(DC.state_of(net_b, opt_b), DC.state_of(net_a, opt_a), "DataParallel against optimize_step")
    assert all(p.grad is None or p.grad.data_ptr() == v.data_ptr()
               for p, v in zip(dp.arena.params, dp.arena.views()))       # the optimiser stepped on the arena
    # a covered parameter without a gradient on a later step
    net_b.conv_first.bias.requires_grad_(False)
    with TR.deterministic(), pytest.raises(RuntimeError, match="received no gradient.*conv_first.bias"):
        dp.step(crit, inputs, gt)


def whole_batch_grads(stif, net, crit, inputs, gt):
    net.zero_grad(set_to_none=True)
    crit(net(*inputs), gt).backward()
    return {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}


def relmax(a, b):
    return float((a - b).abs().max() / a.abs().max())


def tensor_class(key):
    parts = key.split(".")
    return parts[0] + ("." + parts[1] if parts[0] == "ConvBLSTM" else "") + "/" + parts[-1]


def test_the_rank_sum_is_the_gradient_of_the_whole_batch(stif, tmp_path_factory):
    """Sum semantics: the arena of two ranks after step 1 against one process on the batch of 2, per parameter tensor,
    relmax = max|a - b| / max|whole-batch g|.  The yardstick comes from the single-process code alone: the same relmax
    between two whole-batch gradients with the two items swapped (the same per-item terms, added in the other order).
    Allowed: 4 x that (a rank split regroups at most one level deeper than a permutation), floor 2^-20.

    Measured on the MI355X, maxima over the 262 tensors: rank split 2.1e-7, swapped items 3.4e-7 (DESIGN.md section 5
    "Data-parallel training")."""
    TR = stif.train
    res = ranks(tmp_path_factory, 2, TWO_RANKS)[0][0]
    _, _, arena1 = emulated(stif, 2, 2)
    assert DC.same_bytes(res["arena1"], arena1)
    net, _, crit = DC.make_net(stif)
    lq, times, gt = DC.global_batch(2)
    flip = torch.tensor([1, 0], device=lq.device)
    with TR.deterministic():
        whole = whole_batch_grads(stif, net, crit, (lq, times, DC.SHAPE), gt)
        swapped = whole_batch_grads(stif, net, crit, (lq[flip].contiguous(), [t[flip.cpu()] for t in times], DC.SHAPE),
                                    gt[flip].contiguous())
    assert list(whole) == res["names"] and len(whole) == DC.COVERED
    floor, worst, classes = 2.0 ** -20, [], {}
    for k, o, n in zip(res["names"], res["offsets"], res["sizes"]):
        g = whole[k].cpu()
        split = relmax(g, res["arena1"][o:o + n].view_as(g))
        yard = relmax(g, swapped[k].cpu())
        c = classes.setdefault(tensor_class(k), [0.0, 0.0])
        c[0], c[1] = max(c[0], split), max(c[1], yard)
        if split > max(4 * yard, floor):
            worst.append((k, split, yard))
    for name, (split, yard) in sorted(classes.items()):
        print(f"{name:40s} rank split {split:.3e}   swapped items {yard:.3e}")
    print(f"maxima: rank split {max(c[0] for c in classes.values()):.3e}, swapped items "
          f"{max(c[1] for c in classes.values()):.3e}, floor {floor:.3e}")
    assert not worst, worst


OPT = """
name: tiny_ddp
model: VideoSR_base
distortion: sr
scale: 4
datasets:
  train:
    name: Adobe_a
    mode: Adobe_a
    dataroot_GT: {root}
    video_list: {root}/list.txt
    n_workers: 2
    batch_size: 2
    lq_size: 16
network_G:
  which_model_G: LIIF
  nf: 64
  nframes: 7
  groups: 8
  front_RBs: 1
  back_RBs: 1
path:
  pretrain_model_G: ~
  strict_load: true
  resume_state: {resume}
  models: {out}/models
  training_state: {out}/state
train:
  lr_G: !!float 2e-5
  lr_scheme: CosineAnnealingLR_Restart
  beta1: 0.9
  beta2: 0.99
  niter: 3
  warmup_iter: -1
  T_period: [10, 10]
  restarts: [10]
  restart_weights: [1]
  eta_min: !!float 1e-7
  pixel_criterion: cb
  pixel_weight: 1.0
  manual_seed: 0
logger:
  print_freq: 1
  save_checkpoint_freq: {save}
"""


def test_training_script_on_two_ranks_then_resumed_as_one_process(stif, tmp_path):
    tmp = str(tmp_path)
    footage = DC.write_footage(os.path.join(tmp, "footage"))
    out = os.path.join(tmp, "run")
    yml = os.path.join(tmp, "two.yml")
    with open(yml, "w") as f:
        f.write(OPT.format(root=footage, out=out, resume="~", save=2))
    log = _launch(2, ["tools/train.py", "--opt", yml, "--device", "0", "--backend", "gloo", "--deterministic"])
    print(log)
    losses = [float(v) for v in re.findall(r"l_pix: (\S+)", log)]
    assert len(losses) == 3 and all(np.isfinite(v) and v > 0 for v in losses)     # rank 0 alone logs
    assert log.count("saved models and training states at iter 2") == 1 and "end of training" in log
    assert "data-parallel: 2 ranks, backend gloo" in log
    assert sorted(os.listdir(os.path.join(out, "models"))) == ["2_G.pth"]         # and rank 0 alone writes
    assert sorted(os.listdir(os.path.join(out, "state"))) == ["2.state"]
    sd = torch.load(os.path.join(out, "models", "2_G.pth"), map_location="cpu", weights_only=True)
    assert len(sd) == DC.KEYS
    state = torch.load(os.path.join(out, "state", "2.state"), map_location="cpu", weights_only=False)
    assert set(state) == {"epoch", "iter", "schedulers", "optimizers", "seed"} and state["iter"] == 2
    assert len(state["optimizers"][0]["state"]) == DC.COVERED
    # one process resumes the two-rank checkpoint and reaches iteration 3
    yml1 = os.path.join(tmp, "one.yml")
    with open(yml1, "w") as f:
        f.write(OPT.format(root=footage, out=out, resume=os.path.join(out, "state", "2.state"), save=1))
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "train.py"), "--opt", yml1, "--deterministic"],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "resuming training from epoch" in r.stdout and len(re.findall(r"l_pix: (\S+)", r.stdout)) == 1
    sd3 = torch.load(os.path.join(out, "models", "3_G.pth"), map_location="cpu", weights_only=True)
    stif.train.LunaTokis(1, 1).load_state_dict(sd3, strict=True)
    assert not torch.equal(sd3["conv_first.weight"], sd["conv_first.weight"])
    state3 = torch.load(os.path.join(out, "state", "3.state"), map_location="cpu", weights_only=False)
    assert state3["iter"] == 3 and state3["seed"] == state["seed"]
    # the third iteration trained on the same global batch either way: the losses agree to fp32 reassociation
    one = float(re.findall(r"l_pix: (\S+)", r.stdout)[0])
    # Every kernel computes an item independently of the batch it is launched in, so the per-pixel terms are the
    # same bits and only the sums differ: torch.sum's tree over N < 2^15 positive terms is within about
    # log2(N) 2^-24 < 1e-6 of the exact sum on either side, and the log prints seven digits (5e-7).
    print(f"iteration 3: two ranks {losses[2]:.6e}, one process {one:.6e}")
    assert abs(one - losses[2]) <= 1e-5 * abs(one)
