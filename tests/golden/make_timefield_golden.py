"""Generate tests/golden/timefield_16x20.npz: the REFERENCE model's own ``decoding`` with a time per query.

In LunaTokis.decoding the time input is ``pe_coord = ones_like(coord[:, :, 0].unsqueeze(2)) * times[c].unsqueeze(2)``
(Sakuya_arch_test.py:397): a ``times[c]`` of shape [bs, HH*WW] broadcasts there into a different time per query and
every later torch.cat accepts it.  This script sets the reference model's latent (``feat`` / ``inp``) from
model_16x20.npz -- the reference's own gen_feat of that fixture's ``x`` -- and records its decoding for
  * the random four-valued field of tests/timefield_inputs.py at the default 64 x 80, and
  * a row ramp t = y / (HH - 1) at 37 x 45.
Only fields and outputs are written (plain data).  Run by hand where the reference is present, as make_golden.py:

    python tests/golden/make_timefield_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as G  # noqa: E402
import timefield_inputs as TF  # noqa: E402


def main():
    if not os.path.isdir(G.REF):
        print("reference absent; nothing to do")
        return
    model = G._reference_model()
    g = np.load(os.path.join(HERE, "model_16x20.npz"))
    model.feat = torch.from_numpy(g["feat"])[None]          # [1,3,64,16,20]
    model.inp = torch.from_numpy(g["x"])                    # [1,2,3,16,20]
    out = {}
    for name, field, scale in (("random", TF.random_field(1, 64, 80), None), ("ramp", TF.row_ramp(37, 45), (37, 45))):
        _, HH, WW = field.shape
        with torch.no_grad():
            o = model.decoding([torch.from_numpy(field).reshape(1, HH * WW)], scale=scale)[0]
        assert tuple(o.shape) == (1, 3, HH, WW), o.shape
        out[f"{name}_field"] = field.astype(np.float32)
        out[f"{name}_out"] = o.numpy().astype(np.float32)
        print(name, tuple(o.shape), float(o.min()), float(o.max()))
    np.savez_compressed(os.path.join(HERE, "timefield_16x20.npz"), **out)


if __name__ == "__main__":
    main()
