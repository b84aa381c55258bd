"""A functional torch restatement of the reference decoder, LunaTokis.decoding (Sakuya_arch_test.py:364-459), for the
training tests: differentiable (torch autograd gives every gradient the HIP backward is checked against), in float64 or
float32 on the CPU, returning its intermediates, and accepting a given flow for stage 2.

Written from the oracle's documentation of the reference lines (oracle/stif_oracle.py: ``_query_axes``,
``decode_stage1``, ``decode_stage2``), not from the reference's code.  The coordinates are computed in float32 in the
reference's operation order and then cast, exactly as the oracle does, so the float64 run equals the oracle to
rounding (tests/test_dec_train_host.py):

* the query grid is make_coord((HH, WW)) clamped to +-(1 - 1e-6): per axis fp32(-1 + r) + fp32(2 r) * arange(n), r = 1/n;
* the nearest LR index is grid_sample's ``((c + 1) n - 1) / 2`` in float32, rounded half to even, clamped;
* rel_coord = (query - LR pixel centre) * n in float32;
* the bilinear gathers are F.grid_sample(mode='bilinear', padding_mode='zeros', align_corners=False);
* the warped grids are torch.linspace(-1, 1, n) (float32: ``linspace_axis``) + flow / ((n - 1) / 2), clamped to +-(1 - 1e-6).
"""
import numpy as np
import torch
import torch.nn.functional as F

LO = float(np.float32(-1 + 1e-6))
HI = float(np.float32(1 - 1e-6))


def coord_axis(n):
    """One axis of make_coord (:1233-1248) in float32."""
    r = 1.0 / n
    return torch.tensor(-1 + r, dtype=torch.float32) + torch.tensor(2 * r, dtype=torch.float32) * torch.arange(n).float()


def query_axis(n_lr, n_hr):
    """(query coordinate, nearest LR index, rel_coord) of one axis, float32 / int64."""
    q = coord_axis(n_hr).clamp(LO, HI)
    src = ((q + 1) * n_lr - 1) / 2
    near = torch.round(src).long().clamp(0, n_lr - 1)
    rel = (q - coord_axis(n_lr)[near]) * n_lr
    return q, near, rel


def siren(x, sd, p, n_sine):
    for i in range(n_sine):
        x = torch.sin(30.0 * F.linear(x, sd[f"{p}net.{i}.linear.weight"], sd[f"{p}net.{i}.linear.bias"]))
    return F.linear(x, sd[f"{p}net.{n_sine}.weight"], sd[f"{p}net.{n_sine}.bias"])


def bilinear(img, gx, gy):
    """img [B, C, H, W], gx / gy [B, Q] normalised (x along W) -> [B, Q, C]"""
    grid = torch.stack([gx, gy], dim=-1).unsqueeze(1)                     # [B, 1, Q, 2]
    out = F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    return out[:, :, 0, :].permute(0, 2, 1)


def _maps(feat, inp, dtype):
    B = feat.shape[0]
    H, W = feat.shape[-2:]
    return feat.to(dtype).reshape(B, 192, H, W), inp.to(dtype).reshape(B, 6, H, W)


def _time(t, B, Q, dtype):
    return torch.as_tensor(t, dtype=dtype).reshape(-1, 1, 1).expand(B, Q, 1)


def stage1_inputs(feat, inp, t, HH, WW, dtype=torch.float64):
    """X1 [B, Q, 201] and the fixed-grid part of X2 [B, Q, 199] (bilinear latent, bilinear frames, t)."""
    featc, inpc = _maps(feat, inp, dtype)
    B, _, H, W = featc.shape
    Q = HH * WW
    qy, iy, ry = query_axis(H, HH)
    qx, ix, rx = query_axis(W, WW)
    near = (iy[:, None] * W + ix[None, :]).reshape(-1)
    q_feat = featc.reshape(B, 192, H * W)[:, :, near].permute(0, 2, 1)
    q_inp = inpc.reshape(B, 6, H * W)[:, :, near].permute(0, 2, 1)
    rel = torch.stack([ry[:, None].expand(HH, WW), rx[None, :].expand(HH, WW)], -1).reshape(1, Q, 2).to(dtype)
    pe = _time(t, B, Q, dtype)
    x1 = torch.cat([q_feat, q_inp, rel.expand(B, Q, 2), pe], -1)
    gy = qy[:, None].expand(HH, WW).reshape(1, Q).expand(B, Q).to(dtype)
    gx = qx[None, :].expand(HH, WW).reshape(1, Q).expand(B, Q).to(dtype)
    x2_tail = torch.cat([bilinear(featc, gx, gy), bilinear(inpc, gx, gy), pe], -1)
    return x1, x2_tail


def decode_stage1(feat, inp, t, sd, HH, WW, dtype=torch.float64):
    """-> dict(x1 [B,Q,201], hrfeat [B,Q,64], x2 [B,Q,263], flow [B,Q,4])"""
    x1, tail = stage1_inputs(feat, inp, t, HH, WW, dtype)
    hrfeat = siren(x1, sd, "feat_imnet.", 3)
    x2 = torch.cat([hrfeat, tail], -1)      # the HR pixel nearest to an unshifted query is the pixel itself
    return dict(x1=x1, hrfeat=hrfeat, x2=x2, flow=siren(x2, sd, "flow_imnet.", 3))


def linspace_axis(n):
    """torch.linspace(-1, 1, n) in float32 as the reference's device evaluates it (oracle.linspace_f32): a float32
    step, the lower half counted up from -1 and the upper half down from 1."""
    i = torch.arange(n)
    step = torch.tensor(2.0 / (n - 1), dtype=torch.float32)
    return torch.where(i < n // 2, -1.0 + step * i.float(), 1.0 - step * (n - 1 - i).float())


def warp_grids(flow, HH, WW, dtype):
    """The unclamped grids ux, uy [B, Q, 2] (grid 1, grid 2) of flow [B, Q, 4] = (x1, y1, x2, y2) in HR pixels."""
    bx = linspace_axis(WW).to(dtype)[None, :].expand(HH, WW).reshape(1, -1, 1)
    by = linspace_axis(HH).to(dtype)[:, None].expand(HH, WW).reshape(1, -1, 1)
    return bx + flow[..., [0, 2]] / ((WW - 1.0) / 2.0), by + flow[..., [1, 3]] / ((HH - 1.0) / 2.0)


def stage2_inputs(feat, inp, hrfeat, flow, t, HH, WW, dtype=torch.float64):
    """X3 [B, Q, 525] in the oracle's order, and the unclamped grids."""
    featc, inpc = _maps(feat, inp, dtype)
    B = featc.shape[0]
    Q = HH * WW
    hr_img = hrfeat.reshape(B, HH, WW, 64).permute(0, 3, 1, 2)
    ux, uy = warp_grids(flow.reshape(B, Q, 4), HH, WW, dtype)
    gx, gy = ux.clamp(LO, HI), uy.clamp(LO, HI)
    hr = [bilinear(hr_img, gx[..., k], gy[..., k]) for k in range(2)]
    lat = [bilinear(featc, gx[..., k], gy[..., k]) for k in range(2)]
    img = [bilinear(inpc, gx[..., k], gy[..., k]) for k in range(2)]
    return torch.cat(hr + lat + img + [_time(t, B, Q, dtype)], -1), ux, uy


def decode_stage2(feat, inp, hrfeat, flow, t, sd, HH, WW, dtype=torch.float64):
    """-> dict(x3 [B,Q,525], pred [B,3,HH,WW], ux, uy)"""
    x3, ux, uy = stage2_inputs(feat, inp, hrfeat, flow, t, HH, WW, dtype)
    pred = siren(x3, sd, "encode_imnet.", 4)
    return dict(x3=x3, pred=pred.permute(0, 2, 1).reshape(feat.shape[0], 3, HH, WW), ux=ux, uy=uy)


def decoding(feat, inp, times, sd, scale=None, dtype=torch.float64):
    """-> (list of [B,3,HH,WW], list of the per-time intermediates)"""
    B = feat.shape[0]
    H, W = feat.shape[-2:]
    HH, WW = (4 * H, 4 * W) if scale is None else (int(scale[0]), int(scale[1]))
    sd = {k: torch.as_tensor(v).to(dtype) for k, v in sd.items() if "imnet" in k}
    preds, mids = [], []
    for t in times:
        tb = torch.as_tensor(t, dtype=dtype).reshape(-1).expand(B) if not isinstance(t, float) else torch.full((B,), t, dtype=dtype)
        s1 = decode_stage1(feat, inp, tb, sd, HH, WW, dtype)
        s2 = decode_stage2(feat, inp, s1["hrfeat"], s1["flow"], tb, sd, HH, WW, dtype)
        preds.append(s2["pred"])
        mids.append({**s1, **s2})
    return preds, mids


def unnormalise(u, n):
    """grid_sample's pixel coordinate of a normalised one on an axis of n samples."""
    return ((u + 1) * n - 1) / 2


def integer_margin(v):
    """The distance of every element to the nearest integer."""
    return (v - torch.round(v)).abs()
