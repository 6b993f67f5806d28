#!/usr/bin/env python
"""Track points through the frames of a folder (STIR-style point tracking on a
whole sequence, with RAFT's video warm start).

    python track.py --model M [--small --mixed_precision --iters 12 --no_warm_start] \
        [--fb_check [--fb_alpha A1 A2]] [--deltas 1 4 16 inf] [--cache_features] \
        --path demo-frames --points points.txt --out tracks.csv
    python track.py --model M --dense --deltas 1 4 16 inf [--points points.txt] [--labels mask.png [--inpaint R]] \
        [--stabilize] [--overlay image.png] --path demo-frames --out tracks/

``points.txt`` holds one ``x y`` per line, in pixels of the first frame.  The
CSV has a ``frame,point,x,y`` row for every point in every frame (frame 0 holds
the given points).  Frames whose size is no multiple of 8 are replicate-padded
for the model and the positions are reported in the unpadded frame.

``--fb_check`` adds the columns ``fb_err,visible``: the forward-backward error
of the step that led to this row, in pixels, and whether the point passed the
check ``|fw + bw|^2 <= A1 * (|fw|^2 + |bw|^2) + A2`` (frame 0 holds ``0.0000,1``).

``--deltas D ...`` tracks over several time spans at once and lets every point
take the most reliable one, so that a point lost behind an occluder is found
again (``export/multiflow.py: MultiFlowTracker``): growing frame distances,
``inf`` last for the first frame as anchor.  The columns are then
``frame,point,x,y,fb_err,visible,score,delta``: ``score`` the accumulated
forward-backward error of the chain that led here (``inf`` for a lost point)
and ``delta`` the span chosen (0: the anchor, -1: none).

``--cache_features`` encodes every frame once and keeps its features on the
device for the later steps that need them (both trackers); the columns are the
same.

``--dense`` (with ``--deltas``) tracks every pixel of the first frame
(``export/denseflow.py: DenseMultiFlowTracker``) and needs no ``--points``;
``--out`` then names a directory, which receives per frame t the long-term flow
``0 -> t`` as ``flow_TTTT.flo`` and the visibility as the 8-bit image
``visible_TTTT.png`` (255: visible), both cropped back from the padding, with
the flow between unpadded coordinates.  ``--dense`` with ``--points`` writes the
eight-column CSV ``tracks.csv`` into that directory as well, the points read
from the dense field after every step (``DenseMultiFlowTracker.query``);
``fb_err`` and ``delta`` are then those of the pixel nearest to the point.

``--dense --labels mask.png [--splat_footprint {1,2}]`` carries a label image
of the first frame (8- or 16-bit, one channel, the first frame's size) through
the video by forward splatting on the model's device (``ops.forward_splat``:
csrc/forward_splat.hip on the GPU; only the warped labels and the coverage go
to the host, to be written): per
frame t ``labels_TTTT.png``, in the mask's bit depth with 0 where no pixel of
the first frame lands, and ``covered_TTTT.png`` (255: some pixel lands there).
The mask is padded like the frames, with label 0, and the images are cropped
back.  ``--inpaint R`` (an integer or ``inf``; default 0: off) fills the holes
that have a covered cell within R cells with that cell's label
(``ops.splat_inpaint``: csrc/splat_inpaint.hip on the GPU);
``covered_TTTT.png`` then holds 255 where a pixel lands, 128 where the label
was in-painted and 0 at the holes that are left.

``--dense --reanchor_every N`` / ``--reanchor_below F`` re-anchor the tracker on
a later frame when the first one has drifted out of view (every N-th frame, or
once fewer than the fraction F of the current anchor's pixels are visible;
``DenseMultiFlowTracker.reanchor``).  Every file still describes ``0 -> t`` in
the pixels of the first frame; without the options the files are unchanged.

``--dense --stabilize`` writes per frame t ``stab_TTTT.png``, 8-bit RGB: frame t
in the first frame's coordinates, every pixel of the first frame showing what
frame t holds where the pixel went (``DenseMultiFlowTracker.stabilize`` on the
8-bit frame: ``ops.backward_warp``, csrc/backward_warp.hip on the GPU), cropped
back from the padding, 0 where the pixel is not visible or has left the frame.

``--dense --overlay image.png`` takes an 8-bit image of 1, 3 or 4 channels in
the first frame's size (an annotation, a colour overlay; an alpha channel is
warped like the others), pads it with 0 like ``--labels`` and writes per frame
t ``overlay_TTTT.png``: the image carried into frame t, read bilinearly through
the inverse map of the splat (``DenseMultiFlowTracker.warp_image``), which
honours ``--splat_footprint`` and ``--inpaint``; 0 where no pixel of the first
frame lands.  Only what is written goes to the host; without the two options
every other file is unchanged.
"""
import argparse
import csv
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from raft_stir_amd.cli_common import add_model_args, default_device, load_image, load_model  # noqa: E402
from raft_stir_amd.data.frame_utils import writeFlow  # noqa: E402
from raft_stir_amd.export.denseflow import DenseMultiFlowTracker  # noqa: E402
from raft_stir_amd.export.multiflow import MultiFlowTracker  # noqa: E402
from raft_stir_amd.export.pointtrack import SequenceTracker  # noqa: E402
from raft_stir_amd.utils.padder import InputPadder  # noqa: E402


def _deltas(words):
    out = []
    for w in words:
        if w.lower() in ("inf", "none", "anchor"):
            out.append(None)
        else:
            out.append(int(w))
    return tuple(out)


def _radius(word):
    """--inpaint: a radius in cells, or 'inf' for no limit (None)."""
    if word.lower() in ("inf", "none"):
        return None
    r = int(word)
    if not 0 <= r <= 32767:
        raise argparse.ArgumentTypeError(f"a radius in [0, 32767] or 'inf' expected, got {word}")
    return r


def track_multi(args, model, images, pts, dev):
    """--deltas: MultiFlowTracker and the eight-column CSV."""
    tracker = MultiFlowTracker(model, iters=args.iters, deltas=_deltas(args.deltas), fb_alpha=tuple(args.fb_alpha),
                               warm_start=not args.no_warm_start, cache_features=args.cache_features)
    padder = InputPadder(load_image(images[0], dev).shape)
    shift = torch.tensor([padder._pad[0], padder._pad[2]], dtype=torch.float32, device=dev)
    points = torch.from_numpy(pts).to(dev)[None] + shift
    cols = [[], [], [], [], []]
    for t, f in enumerate(images):
        traj = tracker.step(padder.pad(load_image(f, dev))[0], points if t == 0 else None)
        for c, v in zip(cols, (traj, tracker.fb_err, tracker.visible, tracker.score, tracker.delta)):
            c.append(v)
    traj, err, vis, score, delta = (torch.cat(c) for c in cols)
    traj = (traj - shift).cpu().numpy()
    err, vis, score, delta = (v.cpu().numpy() for v in (err, vis, score, delta))
    _write_csv(args.out, traj, err, vis, score, delta)
    print(f"wrote {traj.shape[0]} frames x {traj.shape[1]} points to {args.out}")
    return traj


def _write_csv(path, traj, err, vis, score, delta):
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["frame", "point", "x", "y", "fb_err", "visible", "score", "delta"])
        for t in range(traj.shape[0]):
            for n in range(traj.shape[1]):
                w.writerow([t, n, f"{traj[t, n, 0]:.4f}", f"{traj[t, n, 1]:.4f}", f"{err[t, n]:.4f}", int(vis[t, n]),
                            f"{score[t, n]:.4f}", int(delta[t, n])])


def track_dense(args, model, images, pts, dev):
    """--dense: DenseMultiFlowTracker; a .flo and a visibility image per frame
    in the directory --out, and with --points the eight-column CSV from query()."""
    from PIL import Image
    tracker = DenseMultiFlowTracker(model, iters=args.iters, deltas=_deltas(args.deltas), fb_alpha=tuple(args.fb_alpha),
                                    warm_start=not args.no_warm_start, cache_features=args.cache_features,
                                    reanchor_every=args.reanchor_every, reanchor_below=args.reanchor_below)
    os.makedirs(args.out, exist_ok=True)
    padder = InputPadder(load_image(images[0], dev).shape)
    shift = torch.tensor([padder._pad[0], padder._pad[2]], dtype=torch.float32, device=dev)
    points = None if pts is None else torch.from_numpy(pts).to(dev)[None] + shift
    labels = None
    if args.labels:
        mask = np.asarray(Image.open(args.labels))
        if mask.ndim != 2 or mask.dtype not in (np.uint8, np.uint16):
            raise ValueError(f"{args.labels}: an 8- or 16-bit single-channel PNG expected, got {mask.dtype} "
                             f"{mask.shape}")
        if mask.shape != (padder.ht, padder.wd):
            raise ValueError(f"{args.labels}: the first frame's size {(padder.ht, padder.wd)} expected, got "
                             f"{mask.shape}")
        # the padding carries label 0, not a replicated border
        labels = torch.nn.functional.pad(torch.from_numpy(mask.astype(np.int32)), padder._pad, value=0).to(dev)
    overlay = None
    if args.overlay:
        img = np.asarray(Image.open(args.overlay))
        if img.dtype != np.uint8 or img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] not in (1, 3, 4)):
            raise ValueError(f"{args.overlay}: an 8-bit PNG of 1, 3 or 4 channels expected, got {img.dtype} "
                             f"{img.shape}")
        if img.shape[:2] != (padder.ht, padder.wd):
            raise ValueError(f"{args.overlay}: the first frame's size {(padder.ht, padder.wd)} expected, got "
                             f"{img.shape[:2]}")
        # (1,C,H,W); the padding is 0 (transparent where there is an alpha channel), not a replicated border
        chw = torch.from_numpy(img.reshape(padder.ht, padder.wd, -1).copy()).permute(2, 0, 1)
        overlay = torch.nn.functional.pad(chw, padder._pad, value=0)[None].contiguous().to(dev)
    cols = [[], [], [], [], []]
    for t, f in enumerate(images):
        frame = padder.pad(load_image(f, dev))[0]
        tracker.step(frame)
        if args.stabilize:
            # on the 8-bit frame (the values are integers: the conversion is exact), so the file is the uint8 rule's
            stab, _ = tracker.stabilize(frame.to(torch.uint8), fill=0)
            stab = padder.unpad(stab)[0].permute(1, 2, 0).cpu().numpy()
            Image.fromarray(stab).save(os.path.join(args.out, f"stab_{t:04d}.png"))
        if overlay is not None:
            moved, _ = tracker.warp_image(overlay, footprint=args.splat_footprint, inpaint=args.inpaint, fill=0)
            moved = padder.unpad(moved)[0].permute(1, 2, 0).cpu().numpy()
            Image.fromarray(moved[..., 0] if moved.shape[2] == 1 else moved).save(
                os.path.join(args.out, f"overlay_{t:04d}.png"))
        if labels is not None:
            # splatted where the field is; only what is written goes to the host
            if args.inpaint == 0:
                warped, covered = tracker.warp_labels(labels, footprint=args.splat_footprint, fill=0)
                level = padder.unpad(covered)[0, 0].cpu().numpy().astype(np.uint8) * 255
            else:
                # the labels are integers: one gather along the in-painted map, which also tells filled from hole
                src, covered, _, _ = tracker.splat(None, footprint=args.splat_footprint, inpaint=args.inpaint)
                warped = labels.reshape(-1)[src.reshape(-1).long().clamp_(min=0)].reshape(labels.shape)
                warped = torch.where(src[0, 0] >= 0, warped, torch.zeros_like(warped))
                level = torch.where(covered, 255, torch.where(src >= 0, 128, 0)).to(torch.uint8)
                level = padder.unpad(level)[0, 0].cpu().numpy()
            warped = padder.unpad(warped).cpu().numpy().astype(mask.dtype)
            Image.fromarray(warped).save(os.path.join(args.out, f"labels_{t:04d}.png"))
            Image.fromarray(level).save(os.path.join(args.out, f"covered_{t:04d}.png"))
        # a difference of two positions: the padding's shift cancels
        flow = padder.unpad(tracker.flow)[0].permute(1, 2, 0).cpu().numpy()
        vis = padder.unpad(tracker.visible)[0, 0].cpu().numpy()
        writeFlow(os.path.join(args.out, f"flow_{t:04d}.flo"), flow)
        Image.fromarray(vis.astype(np.uint8) * 255).save(os.path.join(args.out, f"visible_{t:04d}.png"))
        if points is not None:
            p, v, s = tracker.query(points)
            H, W = tracker.pos.shape[-2:]
            near = points[0].round().long()
            near = (near[:, 1].clamp(0, H - 1) * W + near[:, 0].clamp(0, W - 1))[None]
            for c, x in zip(cols, (p - shift, tracker.fb_err.view(1, -1).gather(1, near), v, s,
                                   tracker.delta.view(1, -1).gather(1, near))):
                c.append(x)
    print(f"wrote {len(images)} flow fields and visibility maps to {args.out}")
    if labels is not None:
        print(f"wrote {len(images)} warped label images and coverage maps to {args.out}")
    if args.stabilize:
        print(f"wrote {len(images)} stabilised frames to {args.out}")
    if overlay is not None:
        print(f"wrote {len(images)} warped overlays to {args.out}")
    if points is None:
        return None
    traj, err, vis, score, delta = (torch.cat(c).cpu().numpy() for c in cols)
    _write_csv(os.path.join(args.out, "tracks.csv"), traj, err, vis, score, delta)
    print(f"wrote {traj.shape[0]} frames x {traj.shape[1]} points to {os.path.join(args.out, 'tracks.csv')}")
    return traj


def track(args):
    dev = default_device()
    model = load_model(args, dev)
    images = sorted(glob.glob(os.path.join(args.path, "*.png")) + glob.glob(os.path.join(args.path, "*.jpg")))
    if len(images) < 2:
        raise FileNotFoundError(f"at least two frames (*.png, *.jpg) expected in {args.path!r}")
    pts = None
    if args.points:
        pts = np.loadtxt(args.points, dtype=np.float32, ndmin=2)
        if pts.shape[1] != 2:
            raise ValueError(f"{args.points}: one 'x y' per line expected")
    if args.dense:
        return track_dense(args, model, images, pts, dev)
    if args.deltas:
        return track_multi(args, model, images, pts, dev)
    tracker = SequenceTracker(model, iters=args.iters, warm_start=not args.no_warm_start,
                              fb_check=args.fb_check, fb_alpha=tuple(args.fb_alpha),
                              cache_features=args.cache_features)
    padder = InputPadder(load_image(images[0], dev).shape)
    shift = torch.tensor([padder._pad[0], padder._pad[2]], dtype=torch.float32, device=dev)
    points = torch.from_numpy(pts).to(dev)[None] + shift
    frames = (padder.pad(load_image(f, dev))[0] for f in images)
    traj, err, vis = [], [], []
    for t, frame in enumerate(frames):
        traj.append(tracker.step(frame, points if t == 0 else None))
        if args.fb_check:
            err.append(tracker.fb_err)
            vis.append(tracker.visible)
    traj = (torch.cat(traj) - shift).cpu().numpy()  # (T,N,2)
    if args.fb_check:
        err, vis = torch.cat(err).cpu().numpy(), torch.cat(vis).cpu().numpy()  # (T,N)
    with open(args.out, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["frame", "point", "x", "y"] + (["fb_err", "visible"] if args.fb_check else []))
        for t in range(traj.shape[0]):
            for n in range(traj.shape[1]):
                row = [t, n, f"{traj[t, n, 0]:.4f}", f"{traj[t, n, 1]:.4f}"]
                if args.fb_check:
                    row += [f"{err[t, n]:.4f}", int(vis[t, n])]
                w.writerow(row)
    print(f"wrote {traj.shape[0]} frames x {traj.shape[1]} points to {args.out}")
    return traj


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    add_model_args(parser)
    parser.add_argument("--model", help="restore checkpoint")
    parser.add_argument("--path", default="demo-frames", help="folder of frames")
    parser.add_argument("--points", help="text file, one 'x y' per line (required unless --dense)")
    parser.add_argument("--out", default="tracks.csv", help="the CSV to write; with --dense a directory")
    parser.add_argument("--small", action="store_true", help="use small model")
    parser.add_argument("--mixed_precision", action="store_true", help="use mixed precision")
    parser.add_argument("--iters", type=int, default=12)
    parser.add_argument("--no_warm_start", action="store_true", help="start every pair from zero flow")
    parser.add_argument("--fb_check", action="store_true",
                        help="forward-backward check: adds the CSV columns fb_err,visible")
    parser.add_argument("--fb_alpha", type=float, nargs=2, default=[0.01, 0.5], metavar=("A1", "A2"),
                        help="the check's relative and absolute threshold terms")
    parser.add_argument("--deltas", nargs="+", metavar="D",
                        help="track over these frame distances at once ('inf' last: the first frame as anchor) and "
                             "recover lost points: the CSV columns become x,y,fb_err,visible,score,delta")
    parser.add_argument("--cache_features", action="store_true",
                        help="encode every frame once and keep its features for the later steps")
    parser.add_argument("--dense", action="store_true",
                        help="with --deltas: track every pixel of the first frame and write a .flo and a visibility "
                             "image per frame into the directory --out (with --points: tracks.csv there too)")
    parser.add_argument("--labels", metavar="MASK.png",
                        help="with --dense: an 8- or 16-bit single-channel label image of the first frame; every "
                             "frame's labels_TTTT.png and covered_TTTT.png go into the directory --out")
    parser.add_argument("--splat_footprint", type=int, choices=(1, 2), default=2,
                        help="with --labels / --overlay: a pixel claims its nearest cell (1) or every cell it touches "
                             "(2)")
    parser.add_argument("--inpaint", type=_radius, default=0, metavar="R",
                        help="with --labels / --overlay: fill holes from the nearest covered cell within R cells (an "
                             "integer, or 'inf'); covered_TTTT.png then marks in-painted cells with 128")
    parser.add_argument("--stabilize", action="store_true",
                        help="with --dense: write every frame in the first frame's coordinates as stab_TTTT.png")
    parser.add_argument("--overlay", metavar="IMAGE.png",
                        help="with --dense: an 8-bit image of 1, 3 or 4 channels on the first frame; it is carried "
                             "into every frame as overlay_TTTT.png (honours --splat_footprint and --inpaint)")
    parser.add_argument("--reanchor_every", type=int, metavar="N",
                        help="with --dense: make every N-th frame the new anchor; the files still describe 0 -> t")
    parser.add_argument("--reanchor_below", type=float, metavar="F",
                        help="with --dense: re-anchor once fewer than this fraction (0 < F < 1) of the current anchor's "
                             "pixels are visible; reads one scalar from the device per frame")
    args = parser.parse_args(argv)
    if args.dense and not args.deltas:
        parser.error("--dense needs --deltas")
    if (args.reanchor_every is not None or args.reanchor_below is not None) and not args.dense:
        parser.error("--reanchor_every and --reanchor_below need --dense")
    if args.reanchor_every is not None and args.reanchor_every < 1:
        parser.error("--reanchor_every needs a positive N")
    if args.reanchor_below is not None and not 0.0 < args.reanchor_below < 1.0:
        parser.error("--reanchor_below needs 0 < F < 1")
    if args.labels and not args.dense:
        parser.error("--labels needs --dense")
    if (args.stabilize or args.overlay) and not args.dense:
        parser.error("--stabilize and --overlay need --dense")
    if args.inpaint != 0 and not (args.labels or args.overlay):
        parser.error("--inpaint needs --labels or --overlay")
    if not args.dense and not args.points:
        parser.error("the following arguments are required: --points")
    return args


if __name__ == "__main__":
    track(parse_args())
