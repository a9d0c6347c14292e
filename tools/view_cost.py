"""What crop views cost (DESIGN.md section 5 "Crop views"): ViT-B/32 at P = 64 with synthetic weights behind a mini StyleGAN2, one stream,
per-launch events, for V = 0 (off), 1, 4, 8 views: the sum of the clip.* profile rows of a pass (the resize / view kernel included: it is part
of what V multiplies), median of repeated passes after three warm-ups, the whole un-profiled pass, and the ratio tower(V = 8) / (8 tower(V = 0))
— what one pass over P V rows costs against V separate towers.  Needs a GPU.

    python tools/view_cost.py [--out view_cost.json]
"""
import argparse
import json
import os
import sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import glass_models as M
from clip_glass_amd import synth
from clip_glass_amd.engine import Engine

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the figures and the per-launch rows to this JSON file")
args = ap.parse_args()
P, bs, PASSES, VIEWS = 64, 4, 11, (0, 1, 4, 8)
VIT_B32 = (768, 12, 12, 32, 224, 512)
c = M.CONFIGS["mini"]
sd = synth.make_state(synth.stylegan2_g_spec(c["channels"], c["latent"], c["mapping"]), 0)
sd.update(synth.make_state(synth.clip_visual_spec(VIT_B32[0], VIT_B32[1], VIT_B32[3], VIT_B32[4], VIT_B32[5]), 0))
x = synth.latents(3, P, c["latent"])
out = dict(P=P, passes=PASSES, views={})
for V in VIEWS:
    e = Engine(c["channels"][::-1], latent_size=c["latent"], mapping_layers=c["mapping"], batch_size=bs, use_discriminator=False, n_obj=1,
               max_pop=P, clip=VIT_B32, noise_mode=1, clip_views=V)
    e.load_state(sd)
    e.finalize()
    e.set_target(synth.normal(1, "t", (VIT_B32[5],)))
    e.set_overlap(0)
    for _ in range(3):
        e.evaluate(x)
    e.set_profiling(1)
    tot, rsz, last = [], [], None
    for _ in range(PASSES):
        e.evaluate(x)
        rows = [r for r in e.profile() if r["name"].startswith("clip.")]
        tot.append(sum(r["total_ms"] for r in rows))
        rsz.append(sum(r["total_ms"] for r in rows if r["name"].startswith(("clip.resize", "clip.views"))))
        last = rows
    e.set_profiling(0)
    un = []
    for _ in range(PASSES):
        e.evaluate(x)
        un.append(e.last_gpu_ms())
    e.close()
    out["views"][str(V)] = dict(
        tower_ms_median=float(np.median(tot)), tower_ms_min=float(min(tot)), tower_ms_max=float(max(tot)), resize_ms_median=float(np.median(rsz)),
        whole_pass_unprofiled_ms_median=float(np.median(un)),
        rows=[dict(name=r["name"], launches=r["launches"], ms=round(r["total_ms"], 4), tflops=round(r["flops"] / max(r["total_ms"], 1e-9) / 1e9, 1),
                   gbs=round(r["bytes"] / max(r["total_ms"], 1e-9) / 1e6, 1)) for r in last])
t = {V: out["views"][str(V)]["tower_ms_median"] for V in VIEWS}
out["ratio_tower_v8_over_8_tower_v0"] = t[8] / (8 * t[0])
out["ratio_tower_v4_over_4_tower_v0"] = t[4] / (4 * t[0])
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
for V in VIEWS:
    print(json.dumps(dict(views=V, **{k: v for k, v in out["views"][str(V)].items() if k != "rows"})))
print(json.dumps({k: v for k, v in out.items() if k.startswith("ratio")}))
for r in out["views"]["8"]["rows"]:
    print(r)
