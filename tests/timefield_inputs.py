"""Time fields for the decoder tests and their oracle (shared by tests/test_timefield_host.py,
tests/test_gpu_timefield.py and tests/golden/make_timefield_golden.py; a plain module, not a fixture).

A field gives every pixel of the HH x WW grid of every item its own query time.  The random field draws each pixel
from four values that are exact in fp32, with a different seed per item, so that neighbouring pixels, rows, columns
and items nearly always differ: a field read at the wrong pixel, row, column or item changes 3 pixels in 4.

The oracle of a field is a composite of the unchanged per-item oracle stages: decode_stage1 depends on a pixel's
own time only, so the field's HRfeat / flow is, per pixel, that of the call with the pixel's value; decode_stage2
gathers HRfeat rows of other pixels, so it is run on the composite HRfeat once per value and selected again."""
import numpy as np

from oracle import stif_oracle as O

F32 = np.float32
VALUES = np.array([0.0, 0.3125, 0.625, 1.0], F32)


def random_field(B, HH, WW, seed=100):
    """[B,HH,WW] fp32, every pixel one of VALUES, item i drawn with seed + i."""
    return np.stack([VALUES[np.random.default_rng(seed + i).integers(0, len(VALUES), (HH, WW))] for i in range(B)])


def row_ramp(HH, WW):
    """[1,HH,WW] fp32, t = y / (HH - 1)."""
    return np.broadcast_to((np.arange(HH, dtype=F32) / F32(HH - 1)).astype(F32)[None, :, None], (1, HH, WW)).copy()


def stage1_per_value(feat, inp, values, sd, HH, WW):
    """{value: (hrfeat [B,HH,WW,64], flow [B,HH,WW,4])} of O.decode_stage1 with that time for every item."""
    B = feat.shape[0]
    return {float(v): O.decode_stage1(feat, inp, np.full(B, v, F32), sd, HH, WW) for v in values}


def select(per_value, field):
    """The composite of per-value arrays [B,HH,WW,C]: pixel (b, y, x) from the array of field[b, y, x]."""
    out = None
    for v, a in per_value.items():
        if out is None:
            out = np.full_like(a, np.nan)
        m = field == F32(v)
        out[m] = a[m]
    assert not np.isnan(out).any(), "the field holds a value without an oracle call"
    return out


def stage1_composite(per_value, field):
    return (select({v: hf[0] for v, hf in per_value.items()}, field),
            select({v: hf[1] for v, hf in per_value.items()}, field))


def stage2_composite(feat, inp, hrfeat, flow, field, sd, HH, WW):
    """[B,3,HH,WW]: O.decode_stage2 on (hrfeat, flow) once per distinct value of the field, each pixel taken from
    the call of its value."""
    B = feat.shape[0]
    per = {float(v): np.moveaxis(O.decode_stage2(feat, inp, hrfeat, flow, np.full(B, v, F32), sd, HH, WW), 1, -1)
           for v in np.unique(field)}
    return np.moveaxis(select(per, field), -1, 1)


def decode_composite(feat, inp, field, sd, HH, WW, per_value=None):
    """(hrfeat, flow, rgb) of the field decode."""
    if per_value is None:
        per_value = stage1_per_value(feat, inp, np.unique(field), sd, HH, WW)
    hrf, flow = stage1_composite(per_value, field)
    return hrf, flow, stage2_composite(feat, inp, hrf, flow, field, sd, HH, WW)
