"""stif_amd: MI355X-native (gfx950) engine for the STIF LunaTokis forward.

Import through ``stif_pkg.load()`` (the directory name is not a Python identifier).
Layout:
  csrc/       HIP kernels (conv, DCN, decoder) + C ABI (include/stif.h) + host packing
  _lib.py     ctypes binding of libstif_hip.so (no fallback: missing library -> error)
  ops.py      torch-buffer wrappers of the C ABI
  packing.py  state dict -> packed kernel weights (pack_model, a pure function)
  model.py    LunaTokis host (reference API: forward / gen_feat / decoding / load_state_dict)
  coords.py   fp32 query-grid tables of the decoder
  weights.py  state-dict spec + deterministic weight generator
  video.py    custom_video_test-style sliding-window driver; streaming renderer (any length, any frame rate)
  y4m.py      YUV4MPEG2 reader / writer (pure host; the device side is ops.yuv_to_rgb / rgb_to_yuv)
  metrics.py  on-device PSNR / SSIM of decoded frames against ground truth (the reference's evaluation loop)
(integration/_ext.py at the repo root is the DCNv2 `_ext` shim over ops.dcn_v2_forward)
  parallel.py frame-pair sharding over ranks
  serving.py  option files, define_G / load_network / VideoSRModel (checkpoint drop-in)
  train.py    Charbonnier loss, the two restart LR schedules, Adam set-up (training drop-ins); trainable
              Conv3x3 / ResidualBlock_noBN / make_trunk on the HIP conv forward, data- and weight-gradient kernels
  data.py     training batches from frame folders: window index, the reference's collate draws, the on-device batch
              builder (stif_build_batch) and its numpy restatement, the prefetching loader (tools/train.py is the loop)
"""
from . import weights  # noqa: F401
from . import coords  # noqa: F401


def __getattr__(name):
    # torch-dependent parts load lazily so that weight/coords utilities work without torch/GPU
    if name in ("ops", "packing", "model", "video", "parallel", "_lib", "serving", "train", "metrics", "y4m", "data"):
        import importlib
        return importlib.import_module(f"{__name__}.{name}")
    if name == "LunaTokis":
        from .model import LunaTokis
        return LunaTokis
    raise AttributeError(name)
