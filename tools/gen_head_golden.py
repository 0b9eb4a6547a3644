"""Writes tests/golden/head_*.npz: the OUTPUTS of the reference's Matcher, PositionEmbeddingSine and get_embedder on the recipes of tests/head_cases.py.

Build container only: imports the reference's package in place, unmodified — pass its checkout with --reference (default: $NERFLOC_REFERENCE).  The fine matcher
imports kornia (two functions) and einops: the real kornia is used where it is installed, otherwise tools/kornia_standin.py; which one produced a file is recorded
in it (`kornia_source`).  Nothing of the reference's program text is copied: the files hold results, the 118 state-dict names and shapes, key lists and the
reference's own fp32-versus-fp64 deviation per tensor (max |fp32 - fp64| / max |fp64|).

Per head case the eval run is made in fp32 and in fp64 and the recipe is REFUSED unless (a) no row of the fp64 score matrix is undecided at 1e-4
(tests/match_ref.py: undecided_rows), (b) both runs select identical pairs and (c) there are at least 8 of them — so the tests may demand the reference's pairs
exactly.  The training run sets every dropout probability of the reference to 0 and stores both losses, fine_err and the fp64 gradients of coarse_loss + fine_loss
with respect to the four inputs of tests/head_cases.py: INPUT_GRADS.

    python tools/gen_head_golden.py --reference /path/to/NeRF-Loc
"""
import argparse
import contextlib
import io
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import head_cases as hc  # noqa: E402
from tests import match_ref as mr  # noqa: E402

EVAL_KEYS = ("i_ids", "j_ids", "b_ids", "score_matrix", "mkps3d", "mkps2d_c", "expec_f", "mkps2d_f")
FLOAT_KEYS = ("score_matrix", "mkps3d", "mkps2d_c", "expec_f", "mkps2d_f")


def load_reference(ref_root):
    try:
        import kornia  # noqa: F401
        source = "kornia " + getattr(kornia, "__version__", "?")
    except ImportError:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import kornia_standin
        kornia_standin.install()
        source = "stand-in (tools/kornia_standin.py)"
    sys.path.insert(0, ref_root)
    from nerf_loc.models import matcher
    from nerf_loc.models.COTR import position_encoding
    from nerf_loc.models.conditional_nerf import utils
    return matcher, position_encoding, utils, source


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):   # the reference's encoders print their type
        return fn(*a, **k)


def rel(a32, a64):
    a64 = np.asarray(a64, dtype=np.float64)
    return float(np.abs(np.asarray(a32, dtype=np.float64) - a64).max() / max(np.abs(a64).max(), 1e-300)) if a64.size else 0.0


def tensors(data, dtype, grads=()):
    out = {}
    for k, v in data.items():
        if isinstance(v, np.ndarray):
            t = torch.from_numpy(v)
            if v.dtype == np.float32:
                t = t.to(dtype)
                if k in grads:
                    t.requires_grad_(True)
            out[k] = t
        else:
            out[k] = v
    return out


def build(ref, c, dtype, fine=True):
    C = c["case"].C
    m = quiet(ref.Matcher, hc.Args, C, C, C, fine_matching=fine)
    state = {k: torch.from_numpy(v) for k, v in c["state"].items()}
    if not fine:
        state = {k: v for k, v in state.items() if k.startswith("coarse_")}
    m.load_state_dict(state, strict=True)
    return m.to(dtype)


def run_eval(ref, c, dtype, fine=True, thr=None):
    m = build(ref, c, dtype, fine).eval()
    if thr is not None:
        m.coarse_matcher.thr = thr
    with torch.no_grad():
        return m, m(tensors(c["data"], dtype))


def run_train(ref, c, dtype):
    m = build(ref, c, dtype).train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
        if isinstance(mod, torch.nn.MultiheadAttention):
            mod.dropout = 0.0
    data = tensors(c["data"], dtype, hc.INPUT_GRADS)
    out = m(data)
    (out["coarse_loss"] + out["fine_loss"]).backward()
    return out, {k: data[k].grad.numpy() for k in hc.INPUT_GRADS}


def shapes_of(out, keys):
    return np.array([",".join(str(s) for s in out[k].shape) if torch.is_tensor(out[k]) else type(out[k]).__name__ for k in keys])


def save(path, **arrays):
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) < (1 << 20), f"{path} is {os.path.getsize(path)} bytes"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("NERFLOC_REFERENCE", ""))
    args = ap.parse_args()
    ref, pe, utils, source = load_reference(args.reference)
    print("kornia:", source)
    torch.set_num_threads(8)
    gdir = hc.golden_dir()

    # ---- position tables: the reference's forward is fp32 by construction (cumsum(dtype=float32)); its fp64 form is its own sine module on the fp64 grid
    for C in hc.POS_CHANNELS:
        mod = quiet(pe.PositionEmbeddingSine, C // 2, normalize=True, sine_type="lin_sine")
        arrays = {}
        for H, W in hc.POS_SHAPES:
            t32 = mod(torch.zeros(1, H, W))[0].numpy()
            ex = (np.arange(1, W + 1, dtype=np.float64) - 0.5) / (W + 1e-6)
            ey = (np.arange(1, H + 1, dtype=np.float64) - 0.5) / (H + 1e-6)
            pos = np.stack(np.broadcast_arrays(ex[None, :], ey[:, None]), axis=-1)
            t64 = mod.sine(torch.from_numpy(np.ascontiguousarray(pos))).numpy()
            assert t32.shape == (H, W, C) and t32.dtype == np.float32
            arrays[f"pos_{H}x{W}"] = t32
            arrays[f"dev_{H}x{W}"] = np.float64(rel(t32, t64))
            if H * W <= 49:
                arrays[f"pos64_{H}x{W}"] = t64
            print(f"pos {H}x{W} C {C}: fp32 vs fp64 {arrays[f'dev_{H}x{W}']:.2e}")
        save(os.path.join(gdir, f"head_pos_c{C}.npz"), **arrays)

    # ---- embedder
    fn, out_dim = utils.get_embedder(hc.EMBED_L, 0, include_input=False)
    arrays = {"out_dim": np.int64(out_dim)}
    for n in (1, 65):
        x = hc.embed_points_input(n)
        e32 = fn(torch.from_numpy(x)).numpy()
        e64 = fn(torch.from_numpy(x).double()).numpy()
        arrays[f"embed_{n}"], arrays[f"embed64_{n}"], arrays[f"dev_{n}"] = e32, e64, np.float64(rel(e32, e64))
        print(f"embed N {n}: fp32 vs fp64 {arrays[f'dev_{n}']:.2e}")
    save(os.path.join(gdir, "head_embed.npz"), **arrays)

    # ---- the head
    for name in hc.GOLDEN_CASES:
        c = hc.make_case(name)
        m, o32 = run_eval(ref, c, torch.float32)
        _, o64 = run_eval(ref, c, torch.float64)
        pairs32 = np.stack([o32["i_ids"].numpy(), o32["j_ids"].numpy()])
        pairs64 = np.stack([o64["i_ids"].numpy(), o64["j_ids"].numpy()])
        und = int(mr.undecided_rows(o64["score_matrix"].numpy(), hc.THR, 1e-4).sum())
        assert und == 0, f"{name}: {und} undecided rows: choose another seed"
        assert pairs32.shape == pairs64.shape and np.array_equal(pairs32, pairs64), f"{name}: fp32 and fp64 select different pairs: choose another seed"
        assert pairs32.shape[1] >= 8, f"{name}: {pairs32.shape[1]} matches: choose another seed"
        sd = m.state_dict()
        assert len(sd) == 118
        arrays = {"state_dict_names": np.array(list(sd.keys())), "state_dict_shapes": np.array([list(v.shape) + [0] * (2 - v.dim()) for v in sd.values()], dtype=np.int64),
                  "kornia_source": np.array(source), "eval_keys": np.array(sorted(set(o32) - set(c["data"])))}
        for k in EVAL_KEYS:
            arrays[k] = o32[k].numpy()
        for k in FLOAT_KEYS:
            arrays[k + "_64"] = o64[k].numpy()
            arrays["dev_" + k] = np.float64(rel(o32[k].numpy(), o64[k].numpy()))
        print(f"{name}: {pairs32.shape[1]} matches ({int((c['planted'][pairs32[0]] == pairs32[1]).sum())} planted); fp32 vs fp64: " +
              ", ".join(f"{k} {arrays['dev_' + k]:.2e}" for k in FLOAT_KEYS))
        # the branches: no match at all (a threshold no score reaches), and the coarse stage alone
        _, m0 = run_eval(ref, c, torch.float32, thr=2.0)
        _, nf = run_eval(ref, c, torch.float32, fine=False)
        for tag, o in (("m0", m0), ("nofine", nf)):
            keys = sorted(set(o) - set(c["data"]))
            arrays[f"{tag}_keys"], arrays[f"{tag}_shapes"] = np.array(keys), shapes_of(o, keys)
        assert len(m0["i_ids"]) == 0 and np.array_equal(nf["i_ids"].numpy(), pairs32[0])
        save(os.path.join(gdir, f"head_{name}.npz"), **arrays)
        # training mode, dropout 0
        t32, _ = run_train(ref, c, torch.float32)
        t64, g64 = run_train(ref, c, torch.float64)
        arrays = {"train_keys": np.array(sorted(set(t32) - set(c["data"])))}
        for k in ("coarse_loss", "fine_loss", "fine_err"):
            arrays[k], arrays[k + "_64"] = np.float32(t32[k].item()), np.float64(t64[k].item())
            arrays["dev_" + k] = np.float64(abs(t32[k].item() - t64[k].item()) / abs(t64[k].item()))
        arrays["expec_f_gt"] = t32["expec_f_gt"].detach().numpy()
        for k in hc.INPUT_GRADS[:3]:
            arrays["grad_" + k] = g64[k]
        print(f"{name} train: " + ", ".join(f"{k} {arrays[k + '_64']:.6f} (fp32 dev {arrays['dev_' + k]:.1e})" for k in ("coarse_loss", "fine_loss", "fine_err")) +
              "; grad maxima " + ", ".join(f"{np.abs(g64[k]).max():.2e}" for k in hc.INPUT_GRADS))
        save(os.path.join(gdir, f"head_{name}_train.npz"), **arrays)
        save(os.path.join(gdir, f"head_{name}_train_map.npz"), grad_feat_fine=g64["feat_fine"])


if __name__ == "__main__":
    main()
