"""Render a YUV4MPEG2 video through LunaTokis: any length, any output frame rate, x`scale` the size.

  python tools/render_video.py in.y4m out.y4m --opt options.yml [--fps-out 60 | --multiplier 8] [--scale 4]
  ffmpeg -i in.mp4 -f yuv4mpegpipe - | python tools/render_video.py - - --opt options.yml --fps-out 60000/1001 \\
      | ffmpeg -i - out.mp4

`-` is stdin / stdout (nothing seeks, so pipes work).  The model comes from a reference-style option file
(``network_G`` + ``path.pretrain_model_G``, stif_amd.serving) or, with --checkpoint, from a state-dict file on the
default LIIF architecture; --seed-weights N uses the deterministic test weights instead (no checkpoint needed).
--scene-threshold X switches the on-device scene-cut detector on (a pair whose cut score exceeds X repeats a real
frame instead of being interpolated; no value is recommended: none has been validated on footage), --hold-pairs
12,340 forces cuts from an edit list; with either, the cut pairs are reported on stderr.
A thin front end of stif_amd.video.render_y4m.
"""
import argparse
import os
import sys
from fractions import Fraction

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stif_pkg  # noqa: E402


def build_model(stif, opt):
    S = stif.serving
    if opt.opt:
        o = S.parse_options(opt.opt)
        model = S.define_G(o)
        path = opt.checkpoint or (o.get("path") or {}).get("pretrain_model_G")
        if not path:
            raise SystemExit("the option file names no path.pretrain_model_G; pass --checkpoint")
        S.load_network(path, model, (o.get("path") or {}).get("strict_load", True))
        return model
    model = stif.LunaTokis(64, 6, 8, 5, 40)
    if opt.checkpoint:
        S.load_network(opt.checkpoint, model, True)
    elif opt.seed_weights is not None:
        model.load_state_dict(stif.weights.make_state_dict(seed=opt.seed_weights), strict=True)
    else:
        raise SystemExit("give --opt, --checkpoint or --seed-weights")
    return model


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("src", help="input .y4m, or - for stdin")
    ap.add_argument("dst", help="output .y4m, or - for stdout")
    ap.add_argument("--opt", help="YAML option file (network_G, path.pretrain_model_G)")
    ap.add_argument("--checkpoint", help="state-dict file (overrides the option file's path)")
    ap.add_argument("--seed-weights", type=int, help="deterministic test weights with this seed")
    ap.add_argument("--fps-out", type=Fraction, help="output frame rate, e.g. 60 or 60000/1001")
    ap.add_argument("--multiplier", type=Fraction, default=Fraction(8), help="output rate = this x the input rate")
    ap.add_argument("--scale", type=float, default=4.0, help="output size = this x the input size")
    ap.add_argument("--size", help="output size WxH instead of --scale")
    ap.add_argument("--chunk-pairs", type=int, default=8, help="frame pairs rendered at a time (bounds the memory)")
    ap.add_argument("--matrix", choices=("auto", "bt601", "bt709"), default="auto")
    ap.add_argument("--scene-threshold", type=float, help="detect scene cuts: hold a frame where the cut score of a "
                    "pair (video.scene_scores, in [0, 1]) exceeds this; off when not given")
    ap.add_argument("--hold-pairs", default="", help="comma-separated pair indices to treat as cuts, e.g. 12,340")
    ap.add_argument("--ensemble", action="store_true", help="decode every frame with the local ensemble (four "
                    "shifted decodes blended per pixel: no seams at LR pixel borders, about four times the decode)")
    opt = ap.parse_args(argv)
    stif = stif_pkg.load()
    model = build_model(stif, opt)
    out_size = None
    if opt.size:
        ow, oh = opt.size.lower().split("x")
        out_size = (int(oh), int(ow))
    hold = [int(p) for p in opt.hold_pairs.split(",") if p.strip()]
    cuts = []
    src = sys.stdin.buffer if opt.src == "-" else opt.src
    dst = sys.stdout.buffer if opt.dst == "-" else opt.dst
    nin, nout = stif.video.render_y4m(model, src, dst, fps_out=opt.fps_out, multiplier=opt.multiplier,
                                      scale=opt.scale, chunk_pairs=opt.chunk_pairs, matrix=opt.matrix,
                                      out_size=out_size, scene_threshold=opt.scene_threshold, hold_pairs=hold,
                                      cuts=cuts, ensemble=opt.ensemble)
    print(f"{nin} frames in, {nout} frames out", file=sys.stderr)
    if opt.scene_threshold is not None or hold:
        print(f"{len(cuts)} cut pairs: {','.join(map(str, cuts))}", file=sys.stderr)


if __name__ == "__main__":
    main()
