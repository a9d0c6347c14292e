"""What the latent spaces and the truncation trick cost (DESIGN.md section 5 "Latent spaces"): StyleGAN2 ffhq 1024 px + D + CLIP ViT-B/32 at
P = 64 with synthetic weights, one process.  Per mode — z, z with psi 0.7, z with psi 0.7 and cutoff 8, w, w+ — the summed profile rows
mapping + dlatents + styles + demod + premod_weights of a single-stream instrumented pass and the whole un-instrumented pass in the default
stream mode, medians of 12 after a warm-up.  Two comparisons:
  * the layered path's `styles` row (z, psi 0.7, cutoff 8) over the single launch_dense `styles` row (z, psi 0.7): same FLOPs;
  * with --parent LIB (a build of the commit before this feature, loaded through GLASS_LIB as tools/layer_ab.py does): z / psi 1 of this
    library against the parent's, interleaved, next to the parent against a second engine of itself — the run-to-run spread.
Also checks that this library's z / psi 1 pass gives the parent's fitness rows bit for bit.  Needs a GPU.

    python tools/latent_mode_cost.py [--parent tools/lib/libglass_parent.so] [--out latent_mode_cost.json]
"""
import argparse
import json
import os
import sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clip_glass_amd import synth
from clip_glass_amd import engine as E

ap = argparse.ArgumentParser()
ap.add_argument("--parent", default=None, help="libglass.so of the parent commit")
ap.add_argument("--out", default=None, help="also write the figures to this JSON file")
ap.add_argument("--pop", type=int, default=64)
ap.add_argument("--passes", type=int, default=12)
ap.add_argument("--mini", action="store_true", help="rehearsal: the 32 px test network instead of ffhq")
args = ap.parse_args()
P, PASSES = args.pop, args.passes
if args.mini:
    ch, L, mp, clip = [16, 16, 32, 32], 32, 2, (64, 2, 1, 8, 32, 32)
else:
    ch, L, mp, clip = synth.FFHQ_CHANNELS, 512, 8, (768, 12, 12, 32, 224, 512)
NL = 2 * len(ch)
ROWS = ("mapping", "dlatents", "styles", "demod", "premod_weights")
sd = synth.make_state(synth.stylegan2_g_spec(ch, L, mp), 0)
sd.update(synth.make_state(synth.stylegan2_d_spec(ch), 0))
sd.update(synth.make_state(synth.clip_visual_spec(clip[0], clip[1], clip[3], clip[4], clip[5]), 0))
avg = synth.dlatent_avg(L, 0)
z = synth.latents(3, P, L).astype(np.float32)


def make(lib_path, **latent):
    E._lib = None
    if lib_path:
        os.environ["GLASS_LIB"] = os.path.abspath(lib_path)
    else:
        os.environ.pop("GLASS_LIB", None)
    e = E.Engine(ch[::-1], latent_size=L, mapping_layers=mp, batch_size=4, use_discriminator=True, n_obj=2, max_pop=P, clip=clip,
                 noise_mode=1, noise_seed=1234, **latent)
    e.load_state(sd)
    if lib_path is None:
        e.load_tensor("dlatent_avg", avg)
    e.finalize()
    e.set_target(np.ones(clip[5], np.float32))
    return e


def head_pass(e, x):
    """(summed rows ms, per-row ms) of one single-stream instrumented pass."""
    e.set_overlap(0)
    e.set_profiling(1)
    e.evaluate(x)
    rows = {r["name"]: r["total_ms"] for r in e.profile() if r["name"] in ROWS}
    e.set_profiling(0)
    e.set_overlap(2)
    return sum(rows.values()), rows


def whole_pass(e, x):
    e.evaluate(x)
    return e.last_gpu_ms()


def med(v):
    return float(np.median(v))


out = dict(P=P, passes=PASSES, network="mini" if args.mini else "ffhq", modes={})
# ---- z / psi 1 against the parent, interleaved -----------------------------------------------------------------------
new = make(None)
w = new.map_latents(z)
engs = [("new", new)]
if args.parent:
    engs += [("parent_a", make(args.parent)), ("parent_b", make(args.parent))]
F = {}
for n, e in engs:
    for _ in range(2):
        F[n] = e.evaluate(z)
    head_pass(e, z)
if args.parent:
    out["z_psi1_rows_bitwise_equal_to_parent"] = bool(np.array_equal(F["new"], F["parent_a"]))
t_head, t_whole = {n: [] for n, _ in engs}, {n: [] for n, _ in engs}
rows_new = []
for _ in range(PASSES):
    for n, e in engs:
        h, rows = head_pass(e, z)
        t_head[n].append(h)
        if n == "new":
            rows_new.append(rows)
# the un-instrumented passes in a loop of their own, behind a warm-up, and in rotating order: a pass that follows an instrumented one, or
# always takes the first slot of a round, is not comparable with one that follows its like
for n, e in engs:
    whole_pass(e, z)
for r in range(PASSES):
    for k in range(len(engs)):
        n, e = engs[(r + k) % len(engs)]
        t_whole[n].append(whole_pass(e, z))
for n, e in engs:
    e.close()
out["modes"]["z"] = dict(head_ms=med(t_head["new"]), whole_ms=med(t_whole["new"]), rows={k: med([r.get(k, 0.0) for r in rows_new]) for k in ROWS})
if args.parent:
    out["parent"] = {n: dict(head_ms=med(t_head[n]), whole_ms=med(t_whole[n]), whole_ms_min=min(t_whole[n]), whole_ms_max=max(t_whole[n]))
                     for n in t_head}
    out["new_minus_parent_whole_ms"] = med(t_whole["new"]) - med(t_whole["parent_a"])
    out["parent_spread_whole_ms"] = abs(med(t_whole["parent_a"]) - med(t_whole["parent_b"]))
    out["new_minus_parent_head_ms"] = med(t_head["new"]) - med(t_head["parent_a"])
    out["parent_spread_head_ms"] = abs(med(t_head["parent_a"]) - med(t_head["parent_b"]))
# ---- the other modes ---------------------------------------------------------------------------------------------------
w_plus = np.tile(w, (1, NL))
for name, x, latent in (("z psi 0.7", z, dict(truncation_psi=0.7)),
                        ("z psi 0.7 cutoff 8", z, dict(truncation_psi=0.7, truncation_cutoff=min(8, NL - 1))),
                        ("w", w, dict(latent_space="w")),
                        ("w+", w_plus, dict(latent_space="w+"))):
    e = make(None, **latent)
    for _ in range(2):
        e.evaluate(x)
    head_pass(e, x)
    hs, rs, ws = [], [], []
    for _ in range(PASSES):
        h, rows = head_pass(e, x)
        hs.append(h)
        rs.append(rows)
    whole_pass(e, x)
    for _ in range(PASSES):
        ws.append(whole_pass(e, x))
    e.close()
    out["modes"][name] = dict(head_ms=med(hs), whole_ms=med(ws), rows={k: med([r.get(k, 0.0) for r in rs]) for k in ROWS})
m = out["modes"]
out["styles_layered_over_single_launch"] = m["z psi 0.7 cutoff 8"]["rows"]["styles"] / m["z psi 0.7"]["rows"]["styles"]
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
print("%-22s %9s %9s   %s" % ("mode", "head ms", "pass ms", "  ".join("%s" % k for k in ROWS)))
for name, v in m.items():
    print("%-22s %9.4f %9.3f   %s" % (name, v["head_ms"], v["whole_ms"], "  ".join("%.4f" % v["rows"][k] for k in ROWS)))
print(json.dumps({k: v for k, v in out.items() if k != "modes"}))
