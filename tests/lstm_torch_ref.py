"""A pure-torch, differentiable reference of Easy_PCD, the ConvLSTM cell, DeformableConvLSTM, BiDeformableConvLSTM and
gen_feat (not a test), built on tests/pcd_torch_ref.py and written from the module structure
(Sakuya_arch_test.py:132-266, :313-362; convlstm.py:42-58): functions of a parameter dict keyed like the state dict, in
whatever dtype the inputs have.  tests/test_lstm_train_host.py pins them to the numpy oracle; the GPU tests compare the HIP modules with them.

Taming the recurrence (``tame_recurrence``): one conv_offset_mask meets a different ``fea`` at every step and in both
directions, and later steps depend on earlier deformable convs, so the one-pass recipe of pcd_torch_ref.tame_offsets is
repeated: run the whole function, rescale the offset rows of every DCN to |offset - 0.5| <= 0.3 over all of its calls,
run again, for a handful of passes (rescaling only ever shrinks the rows, and the band asserted afterwards, [0.1, 0.9],
is wider than the band scaled to).  ``assert_all_tame`` is the check every test makes on the float64 reference before it
compares anything: a failure is an input bug, never a tolerance case."""
import torch
import torch.nn.functional as F

import pcd_torch_ref as R

N_OFF = 2 * R.DG * R.K


class Calls(dict):
    """{DCN name with its prefix: [fea of every call]}: what ``pcd_align`` saw, over a whole recurrence."""

    def add(self, prefix, feas):
        for name, fea in feas.items():
            self.setdefault(prefix + name, []).append(fea.detach())


def sub(P, prefix):
    return {k[len(prefix):]: v for k, v in P.items() if k.startswith(prefix)}


def conv(P, name, x, stride=1):
    w = P[name + ".weight"]
    return F.conv2d(x, w, P[name + ".bias"], stride=stride, padding=w.shape[2] // 2)


def pyramid(P, p, L1):
    L2 = R.lrelu(conv(P, p + "fea_L2_conv2", R.lrelu(conv(P, p + "fea_L2_conv1", L1, 2))))
    L3 = R.lrelu(conv(P, p + "fea_L3_conv2", R.lrelu(conv(P, p + "fea_L3_conv1", L2, 2))))
    return L2, L3


def aligned(P, p, fea1, fea2, calls=None):
    feas = {}
    y = R.pcd_align(sub(P, p), fea1, fea2, feas)
    if calls is not None:
        calls.add(p, feas)
    return y


def easy_pcd(P, p, f1, f2, calls=None):
    B = f1.shape[0]
    L2, L3 = pyramid(P, p, torch.cat([f1, f2], 0))
    y = aligned(P, p + "pcd_align.", [f1, L2[:B], L3[:B]], [f2, L2[B:], L3[B:]], calls)
    return conv(P, p + "fusion", y)


def lstm_gates(pre, c):
    i, f, o, g = torch.split(pre, pre.shape[1] // 4, dim=1)
    c_next = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(c_next), c_next


def conv_lstm_cell(P, p, x, h, c):
    return lstm_gates(conv(P, p + "conv", torch.cat([x, h], 1)), c)


def deformable_conv_lstm(P, p, xs, calls=None):
    """xs: list over time of [B, 64, H, W]; returns the list of hidden states."""
    h = c = torch.zeros_like(xs[0])
    outs = []
    for x in xs:
        h, c = conv_lstm_cell(P, p + "cell_list.0.", x, easy_pcd(P, p + "pcd_h.", x, h, calls),
                              easy_pcd(P, p + "pcd_c.", x, c, calls))
        outs.append(h)
    return outs


def bi_convlstm(P, xs, calls=None, p="ConvBLSTM."):
    fwd = deformable_conv_lstm(P, p + "forward_net.", xs, calls)
    rev = deformable_conv_lstm(P, p + "forward_net.", xs[::-1], calls)[::-1]
    return [conv(P, p + "conv_1x1", torch.cat([a, b], 1)) for a, b in zip(fwd, rev)]


def resblock(P, name, x):
    return x + conv(P, name + ".conv2", F.relu(conv(P, name + ".conv1", x)))


def gen_feat(P, x, front_RBs, back_RBs, calls=None, capture=None):
    """x [B, N, 3, H, W] -> [B, 2N - 1, 64, H, W]."""
    B, N, _, H, W = x.shape
    L1 = R.lrelu(conv(P, "conv_first", x.reshape(B * N, 3, H, W)))
    for i in range(front_RBs):
        L1 = resblock(P, f"feature_extraction.{i}", L1)
    L2, L3 = pyramid(P, "", L1)
    lv = [t.reshape(B, N, 64, t.shape[2], t.shape[3]) for t in (L1, L2, L3)]
    seq = [lv[0][:, 0]]
    for i in range(N - 1):
        y = aligned(P, "pcd_align.", [t[:, i] for t in lv], [t[:, i + 1] for t in lv], calls)
        seq += [conv(P, "fusion", y), lv[0][:, i + 1]]
    feats = torch.stack(bi_convlstm(P, seq, calls), 1)
    if capture is not None:
        capture["bilstm"] = feats
    out = feats.reshape(B * len(seq), 64, H, W)
    for i in range(back_RBs):
        out = resblock(P, f"recon_trunk.{i}", out)
    return out.reshape(B, len(seq), 64, H, W)


# ---- parameters ----

def conv_shapes(name, cout, cin, k=3):
    return {name + ".weight": (cout, cin, k, k), name + ".bias": (cout,)}


def easy_pcd_shapes(p=""):
    s = {}
    for n in ("fea_L2_conv1", "fea_L2_conv2", "fea_L3_conv1", "fea_L3_conv2"):
        s.update(conv_shapes(p + n, 64, 64))
    s.update({p + "pcd_align." + k: v for k, v in R.pcd_param_shapes().items()})
    s.update(conv_shapes(p + "fusion", 64, 128, 1))
    return s


def bilstm_shapes(p="ConvBLSTM."):
    """{state-dict key: shape} of BiDeformableConvLSTM in the reference's registration order."""
    s = conv_shapes(p + "forward_net.cell_list.0.conv", 256, 128)
    s.update(easy_pcd_shapes(p + "forward_net.pcd_h."))
    s.update(easy_pcd_shapes(p + "forward_net.pcd_c."))
    s.update(conv_shapes(p + "conv_1x1", 64, 128, 1))
    return s


def gen_feat_shapes(front_RBs, back_RBs):
    s = conv_shapes("conv_first", 64, 3)
    for i in range(front_RBs):
        s.update(conv_shapes(f"feature_extraction.{i}.conv1", 64, 64))
        s.update(conv_shapes(f"feature_extraction.{i}.conv2", 64, 64))
    for n in ("fea_L2_conv1", "fea_L2_conv2", "fea_L3_conv1", "fea_L3_conv2"):
        s.update(conv_shapes(n, 64, 64))
    s.update({"pcd_align." + k: v for k, v in R.pcd_param_shapes().items()})
    s.update(conv_shapes("fusion", 64, 128, 1))
    s.update(bilstm_shapes())
    for i in range(back_RBs):
        s.update(conv_shapes(f"recon_trunk.{i}.conv1", 64, 64))
        s.update(conv_shapes(f"recon_trunk.{i}.conv2", 64, 64))
    return s


def random_params(shapes, seed):
    """Float64 parameters: uniform weights of variance 1 / fan_in (every layer keeps the size of its input), biases in
    +-0.1 -- the rule of pcd_torch_ref.random_pcd_params."""
    g = torch.Generator().manual_seed(seed)
    P = {}
    for k, shp in shapes.items():
        bound = 0.1 if len(shp) == 1 else (3.0 / (shp[1] * shp[2] * shp[3])) ** 0.5
        P[k] = (torch.rand(shp, generator=g, dtype=torch.float64) * 2 - 1) * bound
    return P


# ---- the taming recipe over a recurrence ----

def _raw_offsets(P, name, fea):
    return F.conv2d(fea.double(), P[name + ".conv_offset_mask.weight"][:N_OFF].double(), None, padding=1)


def tame_recurrence(P, run, passes=6, margin=0.3):
    """In place on the float64 dict ``P``: ``run(calls)`` evaluates the function under test and records every DCN call;
    each pass sets the offset biases to 0.5 and shrinks the offset rows of every DCN whose offsets leave
    |offset - 0.5| <= margin on any of its calls.  Stops when a pass changes nothing."""
    for _ in range(passes):
        calls = Calls()
        with torch.no_grad():
            run(calls)
            changed = False
            for name, feas in calls.items():
                b = P[name + ".conv_offset_mask.bias"]
                if not bool((b[:N_OFF] == 0.5).all()):
                    b[:N_OFF] = 0.5
                    changed = True
                worst = max(float(_raw_offsets(P, name, fea).abs().max()) for fea in feas)
                if worst > margin:
                    P[name + ".conv_offset_mask.weight"][:N_OFF] *= 0.999 * margin / worst
                    changed = True
        if not changed:
            break
    return calls


def assert_all_tame(P, run):
    """Every fractional offset of every DCN call of ``run`` lies in [0.1, 0.9] on the float64 reference."""
    calls = Calls()
    with torch.no_grad():
        run(calls)
    assert calls
    for name, feas in calls.items():
        for fea in feas:
            offset, _ = R.offset_mask(fea, P[name + ".conv_offset_mask.weight"], P[name + ".conv_offset_mask.bias"])
            R.assert_offsets_tame(offset)
    return calls
