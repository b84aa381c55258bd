"""The cases decoder stage 1 is pinned at (shared by tests/test_oracle.py and tests/test_gpu_decoder_stages.py; a plain
module, not a fixture): a case is (grid, image, shift) -- the HR grid (HH, WW) over the 16 x 20 latent, whether the
flow stage samples decoding_test's x4 HR image instead of the LR pair, and the local ensemble's shift (None: the
whole-grid form, where the flow stage reads the pixel's own HRfeat)."""

T_ITEMS = [0.3, 0.7]                          # a different time per item
LR = (16, 20)                                 # the latent's grid
# 37 x 45: 1665 pixels per item, so a 128-pixel workgroup straddles the items and the last one is partial, and the
# 2.3125 / 2.25 scale has round-half-even ties; 64 x 80: the x4 grid the HR image is made for
GRIDS = [(37, 45), (64, 80)]
# one-row-pair / one-column-triple strips, a downscale, scale 1 (rel ~ 0, every nearest index the pixel itself)
EDGE_GRIDS = [(2, 97), (61, 3), (7, 9), (16, 20)]
SHIFTS = [(-1, -1), (-1, 1), (1, -1), (1, 1)]

WHOLE = [(g, image, None) for g in GRIDS for image in (False, True)] + [(g, False, None) for g in EDGE_GRIDS]
ENSEMBLE = ([((37, 45), False, s) for s in SHIFTS] + [((7, 9), False, (1, -1))]
            + [((64, 80), True, s) for s in ((-1, 1), (1, -1))])
CASES = WHOLE + ENSEMBLE


def case_id(case):
    (HH, WW), image, shift = case
    return f"{'hrimg' if image else 'lr'}-{HH}x{WW}" + ("" if shift is None else f"-shift{shift[0]:+d}{shift[1]:+d}")
