"""Timing of the appearance-adaptation stage at the shipped size: one 480 x 640 frame with ten support views — conv1 11 x 64 x 240 x 320, the coarse map
10 x 60 x 80 x 192, the fine map 10 x 120 x 160 x 192, with --rgb the images 10 x 480 x 640 x 3.

    python tools/appearance_bench.py [--out profiles/appearance_bench.jsonl] [--reps 30] [--rgb] [--channels-last]

The stage is what NerfPoseEstimator.appearance_adaptation does: two embeddings (query, supports) and two adapt layers (three with --rgb).  Every comparison is
the library path against the SAME module's eager formulation (hip_eval / hip_training = False) in the same process on the same tensors, eager timed before and
after the library; the eager embedding is one batched torch.std_mean, which is faster than the reference's loop over the images.  JSON lines, APPENDED to --out:
  what = "stage_eval" / "stage_train"   the whole stage, forward in eval mode / forward + backward in training mode (the maps and all parameters want gradients)
  what = "piece_eval" / "piece_train"   one module alone (embedding, coarse layer, fine layer, rgb layer): these decide each piece's default
  what = "entry"                        one entry point alone: ms per call from device events around `--chain` back-to-back calls, the bytes the algorithm has to
                                        move (computed from the shapes: maps read + maps written), bytes / time, and that rate over the 6.29 TB/s of a float4 copy
ms_* are device-event times of single steps after warm-up, each started on an idle device (median / min / max; launch latency and host work are inside: the
steps are short enough to be bound by them); `spread_ms` is |eager before - eager after|; device_ms_* is the same step queued behind ~10 ms of other work, so that
the host is ahead and the step's kernels run back to back (what a training step with a busy queue sees).  An entry's bytes / time can exceed
the HBM rate where its maps fit in the 256 MiB Infinity Cache between calls (the coarse map does); the line says so (`fits_infinity_cache`).
Needs a HIP device: a timing taken elsewhere says nothing.  Run it under a time limit of its own (the whole run is well under two minutes).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nerf_loc_amd import _app_lib  # noqa: E402
from nerf_loc_amd.appearance import AppearanceAdaptLayer, AppearanceEmbedding  # noqa: E402
from tests import appearance_cases as ac  # noqa: E402
from tools.match_train_bench import timed  # noqa: E402

COPY_TBS = 6.29   # MI355X, float4 copy, measured (the microarchitecture notes' HBM table)
V = 10
SHAPES = {"conv1": (V + 1, 64, 240, 320), "coarse": (V, 60, 80, 192), "fine": (V, 120, 160, 192), "rgb": (V, 480, 640, 3)}


def stats(ms):
    return {"ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms)), "timed": len(ms)}


def timed_behind(fn, reps, busy):
    """Device time of fn's work with the host AHEAD of the device, as inside a training step whose queue the backbone keeps full: a kernel of several milliseconds
    is queued first, so fn's launches are all enqueued before the first of them starts and the events bracket kernels that run back to back."""
    ms = []
    for _ in range(reps):
        busy()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def compare(what, name, make_fn, reps, warmup, extra, busy):
    """make_fn(library: bool) -> a step; eager before, library, eager after.  ms_*: a step timed on its own from an idle device (launch latency and host work
    included: these steps are short enough to be bound by them); device_ms_*: the same step behind a busy device (timed_behind)."""
    eager, lib = make_fn(False), make_fn(True)
    before = timed(eager, reps, warmup)
    mine = timed(lib, reps, warmup)
    after = timed(eager, reps, 1)
    dev_e, dev_l = timed_behind(eager, max(reps // 2, 5), busy), timed_behind(lib, max(reps // 2, 5), busy)
    b, a = float(np.median(before)), float(np.median(after))
    de, dl = float(np.median(dev_e)), float(np.median(dev_l))
    e = dict(what=what, name=name, path="eager", **stats(before + after), ms_median_before=b, ms_median_after=a, spread_ms=abs(b - a), device_ms_median=de,
             device_ms_min=float(np.min(dev_e)), **extra)
    m = stats(mine)
    line = dict(what=what, name=name, path="library", **m, eager_over_library=e["ms_median"] / m["ms_median"],
                faster_beyond_spread=bool(m["ms_median"] + abs(b - a) < min(b, a)), device_ms_median=dl, device_ms_min=float(np.min(dev_l)),
                eager_over_library_device=de / dl, **extra)
    return [e, line]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "appearance_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chain", type=int, default=10)
    ap.add_argument("--rgb", action="store_true")
    ap.add_argument("--channels-last", action="store_true", help="conv1 as a channels_last tensor (what a channels-last backbone hands over)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("appearance_bench.py needs a HIP device: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(5)
    conv1 = torch.relu(torch.randn(SHAPES["conv1"], device=dev, generator=gen))
    if args.channels_last:
        conv1 = conv1.contiguous(memory_format=torch.channels_last)
    names = ["coarse", "fine"] + (["rgb"] if args.rgb else [])
    maps = {n: (torch.rand(SHAPES[n], device=dev, generator=gen) if n == "rgb" else torch.randn(SHAPES[n], device=dev, generator=gen)) for n in names}
    g_ys = {n: torch.randn(SHAPES[n], device=dev, generator=gen) for n in names}
    rng = np.random.default_rng(7)
    states = {n: ac.make_state(SHAPES[n][3], rng) for n in names}
    extra = {"rgb": args.rgb, "conv1_layout": "channels_last" if args.channels_last else "nchw", "views": V}

    def embedding(library):
        m = AppearanceEmbedding(ac.Args())
        m.hip_eval = library
        return m

    def layer(n, library):
        m = AppearanceAdaptLayer(ac.Args(), SHAPES[n][3], is_rgb=n == "rgb")
        m.load_state_dict({k: torch.from_numpy(v) for k, v in states[n].items()}, strict=True)
        m.hip_eval = m.hip_training = library
        return m.to(dev)

    def embeddings_of(emb):
        with torch.no_grad():   # conv1 is frozen in the reference: never differentiated
            return emb(None, {"conv1": conv1[:1]}), emb(None, {"conv1": conv1[1:]})

    def eval_stage(library, only=None):
        emb = embedding(library)
        layers = {n: layer(n, library).eval() for n in names}

        def step():
            with torch.no_grad():
                target, support = embeddings_of(emb)
                return [layers[n](maps[n], support, target) for n in names if only in (None, n)]
        return step

    def train_stage(library, only=None):
        emb = embedding(library)
        layers = {n: layer(n, library).train() for n in names}
        leaves = {n: maps[n].clone().requires_grad_(True) for n in names}

        def step():
            target, support = embeddings_of(emb)
            for n in names:
                if only in (None, n):
                    layers[n].zero_grad(set_to_none=True)
                    leaves[n].grad = None
                    layers[n](leaves[n], support, target).backward(g_ys[n])
            return [leaves[n].grad for n in names if only in (None, n)]
        return step

    def emb_only(library):
        emb = embedding(library)
        return lambda: embeddings_of(emb)

    big = torch.randn((8192, 8192), device=dev, generator=gen)
    big_out = torch.empty_like(big)
    busy = lambda: torch.mm(big, big, out=big_out)   # ~10 ms of fp32 matmul: longer than any step's host time

    lines = []
    # what is timed computes the same thing
    for a, b in zip(eval_stage(True)(), eval_stage(False)()):
        extra.setdefault("eval_max_rel_diff_vs_eager", []).append(float(((a - b).abs().max() / b.abs().max()).item()))
    for a, b in zip(train_stage(True)(), train_stage(False)()):
        extra.setdefault("train_grad_max_rel_diff_vs_eager", []).append(float(((a - b).abs().max() / b.abs().max()).item()))
    lines += compare("stage_eval", "stage", eval_stage, args.reps, args.warmup, extra, busy)
    lines += compare("stage_train", "stage", train_stage, args.reps, args.warmup, extra, busy)
    lines += compare("piece_eval", "embedding", emb_only, args.reps, args.warmup, extra, busy)
    for n in names:
        # a layer alone still needs the embeddings: both paths pay the same library-or-eager embedding, reported above; here the difference is the layer's
        lines += compare("piece_eval", n + " (with embeddings)", lambda lib, n=n: eval_stage(lib, n), args.reps, args.warmup, extra, busy)
        lines += compare("piece_train", n + " (with embeddings)", lambda lib, n=n: train_stage(lib, n), args.reps, args.warmup, extra, busy)

    # entry points alone
    def entry(name, fn, nbytes):
        def chain():
            for _ in range(args.chain):
                fn()
        ms = [t / args.chain for t in timed(chain, max(args.reps // 3, 5), 2)]
        med = float(np.median(ms))
        tbs = nbytes / (med * 1e-3) / 1e12
        lines.append(dict(what="entry", name=name, **stats(ms), calls_per_timing=args.chain, bytes=int(nbytes), tb_per_s=tbs, share_of_float4_copy=tbs / COPY_TBS,
                          fits_infinity_cache=bool(nbytes < 256 * 2 ** 20), **extra))

    with torch.no_grad():
        nb = lambda t: t.numel() * 4
        entry("nla_channel_stats conv1 (11 images)", lambda: _app_lib.channel_stats(conv1), nb(conv1))
        entry("nla_channel_stats conv1 (1 image)", lambda: _app_lib.channel_stats(conv1[:1]), nb(conv1[:1]))
        other = conv1.contiguous() if args.channels_last else conv1.contiguous(memory_format=torch.channels_last)
        entry("nla_channel_stats conv1 (11 images, the other layout: " + ("nchw" if args.channels_last else "channels_last") + ")",
              lambda: _app_lib.channel_stats(other), nb(other))
        emb = embedding(True)
        target, support = embeddings_of(emb)
        for n in names:
            m = layer(n, True)
            w = [p.detach() for p in m.mlp.parameters()]
            entry(f"nla_adapt_code {n}", lambda: _app_lib.adapt_code(support, target.reshape(-1), w), 0)
            code = _app_lib.adapt_code(support, target.reshape(-1), w)
            x, g = maps[n], g_ys[n]
            y, gx = torch.empty_like(x), torch.empty_like(x)
            clip = n == "rgb"
            entry(f"nla_film {n}", lambda: _app_lib.film(x, code, clip, out=y), 2 * nb(x))
            entry(f"nla_film_backward {n} (g_x and g_code)", lambda: _app_lib.film_backward(x, code, g, clip, g_x_out=gx), 3 * nb(x))
            entry(f"nla_film_backward {n} (g_x alone)", lambda: _app_lib.film_backward(x, code, g, clip, want_code=False, g_x_out=gx), 3 * nb(x))
            entry(f"torch a * x + b {n} (two kernels, for scale)", lambda: torch.add(torch.mul(x, code[:, None, None, :x.shape[3]], out=y), code[:, None, None, x.shape[3]:], out=y),
                  4 * nb(x))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for line in lines:
            print(json.dumps(line), flush=True)
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
