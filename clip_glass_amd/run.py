"""CLI — mirror of /root/reference/run.py (same flags and outputs) on the HIP engine.

    python -m clip_glass_amd.run --config StyleGAN2_ffhq_d --target "a wolf at night ..." \\
        --generations 50 --tmp-folder ./tmp [--weights synthetic:0 --clip-weights synthetic:0]

The search runs on the native GA / NSGA-II driver in search.py (pymoo 0.4.2.1 does not import under numpy >= 1.24).
Outputs (run.py:29-51, 79-125): genetic-it-*.{jpg,txt} every --save-each generations,
genetic_result (pickle: X, F, G, CV), F.jpg (Pareto scatter, two objectives), ls_result, output.{jpg,txt}.
"""
import argparse
import os
import pickle

import numpy as np

from .config import get_config
from .engine import LATENT_SPACES
from .engine import PROMPT_MODES
from .generator import (CLIP_MODELS, CLIP_PREPROCESS, CLIP_RESNET_MODELS, edit_options, island_options, latent_options, lpips_options,
                        parse_weighted, prompt_options, search_options)
from .operators import get_operators
from .problem import GenerationProblem
from . import search


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--device", type=str, default="cuda")                       # run.py:17
    p.add_argument("--config", type=str, default="StyleGAN2_ffhq_d")
    p.add_argument("--generations", type=int, default=500)
    p.add_argument("--save-each", type=int, default=50)
    p.add_argument("--tmp-folder", type=str, default="./tmp")
    p.add_argument("--target", type=str, default="a wolf at night with the moon in the background")
    # additions (no checkpoints / vocab in this environment)
    p.add_argument("--weights", type=str, default=None, help="directory with G.pth/D.pth, or synthetic:<seed>")
    p.add_argument("--clip-weights", type=str, default=None,
                   help="a CLIP checkpoint (ViT-B-32.pt, ViT-B-16.pt, ViT-L-14.pt, RN50.pt, RN101.pt ...: the tower and its geometry are read from it), "
                        "or synthetic:<seed>")
    p.add_argument("--clip-model", type=str, default=None, choices=sorted(CLIP_MODELS),
                   help="CLIP image tower: selects the geometry of synthetic weights (default ViT-B/32); with a checkpoint it must "
                        "agree with what the checkpoint holds")
    p.add_argument("--clip-resnet", type=str, default=None, choices=sorted(CLIP_RESNET_MODELS),
                   help="CLIP ResNet image tower instead of a ViT: selects the geometry of synthetic weights; with a checkpoint (RN50.pt, "
                        "RN101.pt: detected by their keys) it must agree with what the checkpoint holds.  Not together with --clip-model")
    p.add_argument("--clip-preprocess", type=str, default=None, choices=list(CLIP_PREPROCESS),
                   help="how a generated image is prepared for CLIP: reference (default: the reference's point-sampled bilinear resize, no "
                        "normalisation), antialias (antialiased bilinear resize), clip (CLIP's own transform: antialiased bicubic resize + "
                        "mean / std normalisation — departs from the reference on purpose)")
    p.add_argument("--clip-views", type=int, default=None,
                   help="score each image as the mean similarity over N views: the whole image and N - 1 random crops, the same for every "
                        "candidate of a generation (0, the default: the reference's single whole-image score — this departs from it on purpose)")
    p.add_argument("--clip-view-min", type=float, default=None, help="smallest crop side as a fraction of the image side (default 0.5)")
    p.add_argument("--no-clip-view-flip", dest="clip_view_flip", action="store_false", default=None,
                   help="never mirror a crop (default: each crop is mirrored with probability 1/2)")
    p.add_argument("--clip-view-fixed", action="store_true", default=None, help="the same crops in every generation (default: redrawn per generation)")
    p.add_argument("--latent-space", type=str, default=None, choices=list(LATENT_SPACES),
                   help="StyleGAN2 configs: what the search varies — z (default: the reference's search, through the mapping network), w (the "
                        "dlatent itself), w+ (one dlatent per style layer) or sub (coefficients of the principal directions of W, per group of "
                        "style layers: --subspace-*).  w / w+ / sub depart from the reference's run.py on purpose")
    p.add_argument("--subspace-components", type=int, default=None,
                   help="with --latent-space sub: directions per group of style layers (default 64, capped at the dlatent's size)")
    p.add_argument("--subspace-layers", type=str, default=None, metavar="SPEC",
                   help="with --latent-space sub: comma-separated inclusive ranges of style layers, one group of coefficients per range "
                        "(\"0-3,4-7,8-17\"); layers not named keep the base's dlatent.  Default: one group of every layer")
    p.add_argument("--subspace-samples", type=int, default=None,
                   help="with --latent-space sub: rows of z the mapping network is probed with for the PCA (default 4096)")
    p.add_argument("--subspace-basis", type=str, default=None, metavar="FILE.npz",
                   help="with --latent-space sub: use this basis (mean, components, stdev[, layer_group]: the subspace.npz of an earlier run, "
                        "or a GANSpace export) instead of probing the mapping network")
    p.add_argument("--truncation-psi", type=float, default=None,
                   help="StyleGAN2 configs: the truncation trick, dlatents pulled towards the average dlatent; in [0, 1], 1 (default) is off")
    p.add_argument("--truncation-cutoff", type=int, default=None,
                   help="StyleGAN2 configs: truncate only the style layers below this index (default: every layer)")
    p.add_argument("--lpips-target", type=str, default=None,
                   help="an image to stay close to: adds the LPIPS-VGG16 distance between each generated image and this one as a search "
                        "objective (off by default — the reference's run.py has no such objective; this departs from it on purpose)")
    p.add_argument("--lpips-size", type=int, default=None, help="side the images are area-downscaled to in front of VGG16 (default 256)")
    p.add_argument("--lpips-lambda", type=float, default=None,
                   help="0 (default): the distance is an objective of its own (NSGA-II); > 0: it is added to the similarity objective, times lambda")
    p.add_argument("--lpips-weights", type=str, default=None,
                   help="a torch file with torchvision's vgg16 features.N.{weight,bias} and LPIPS's lin.K.weight, or synthetic:<seed>")
    p.add_argument("--prompt", action="append", default=None, metavar="TEXT[::WEIGHT]",
                   help="one more text prompt next to --target, repeatable; a negative weight steers away from it (\"glasses::-0.5\").  Off by "
                        "default — the reference's run.py has one target; this departs from it on purpose")
    p.add_argument("--image-prompt", action="append", default=None, metavar="PATH[::WEIGHT]",
                   help="a picture as a prompt, repeatable: centre-cropped, resized to the generator's side and encoded as a generated image is")
    p.add_argument("--target-weight", type=float, default=None, help="weight of --target within the prompt set (default 1)")
    p.add_argument("--prompt-mode", type=str, default=None, choices=list(PROMPT_MODES),
                   help="sum (default): the prompts blend into the one similarity objective, sum_t w_t sim_t / sum_t |w_t|; pareto: one objective "
                        "per prompt (2 to 4, NSGA-II)")
    p.add_argument("--edit-image", type=str, default=None,
                   help="edit this picture: the similarity becomes directional — how the generated image moved away from this one against how "
                        "--target moved away from --source-text (off by default; the reference's run.py has no such objective: this departs from "
                        "it on purpose)")
    p.add_argument("--edit-latent", type=str, default=None,
                   help="StyleGAN2 configs: a .npy with one row of the current latent space.  Its generated image is the source of the directional "
                        "similarity, the row is the latent anchor, and generation 0 starts at it")
    p.add_argument("--source-text", type=str, default=None, help="what the source image shows (required with --edit-image / --edit-latent)")
    p.add_argument("--anchor-lambda", type=float, default=None,
                   help="with --edit-latent.  0 (default): the mean squared distance to the source's dlatents is an objective of its own (NSGA-II); "
                        "> 0: it is added to the similarity objective, times lambda")
    p.add_argument("--edit-sigma", type=float, default=None,
                   help="with --edit-latent: spread of generation 0 around the source row (default 0.1; row 0 is the source itself)")
    p.add_argument("--bpe-path", type=str, default=None)
    p.add_argument("--pop-size", type=int, default=None)
    p.add_argument("--stochastic", action="store_true", default=None,
                   help="GPT2 config: top-k temperature sampling instead of greedy decoding (the config table's `stochastic`)")
    p.add_argument("--device-search", action="store_true", default=None,
                   help="StyleGAN2 and BigGAN configs, one rank: keep the population on the GPU and run selection, crossover, mutation (on a "
                        "BigGAN row: SBX / polynomial mutation on z, half-uniform crossover / bit-flip on the class bits), duplicate flags and "
                        "survival there between the passes (off by default: the host search of search.py; refused for GPT2 and with --dist)")
    p.add_argument("--islands", type=int, default=None,
                   help="with --device-search: K populations of --pop-size rows each in one engine and one pass per generation, island i under "
                        "seed + i (off by default: one population; refused for GPT2, with --dist and with --algorithm cmaes)")
    p.add_argument("--migrate-every", type=int, default=None,
                   help="with --islands: every M generations the best rows of island i - 1 replace the worst of island i (default 0: never)")
    p.add_argument("--migrants", type=int, default=None, help="with --migrate-every: rows per migration, 1 (default) .. pop-size / 2")
    p.add_argument("--island-prompt", action="append", default=None, metavar="TEXT",
                   help="repeatable: --target is island 0's prompt and each TEXT adds an island that searches it alone, all in the one pass "
                        "(--islands, if given, must agree; not with migration, --prompt-mode pareto or an edit source)")
    p.add_argument("--algorithm", type=str, default=None, choices=["ga", "nsga2", "cmaes"],
                   help="the search rule (default: the config's own — nsga2 with the discriminator, ga without).  cmaes: separable CMA-ES, one "
                        "objective and real-valued rows (the StyleGAN2 _nod configs, in z, w, w+ or sub; an LPIPS / anchor distance folded in with "
                        "lambda > 0); with --device-search its generation step runs on the GPU.  Off by default — the reference has GA / NSGA-II")
    p.add_argument("--cma-sigma", type=float, default=None,
                   help="with --algorithm cmaes: the initial step size (default 1: in z, generation 0 is then drawn from the reference's own "
                        "N(0, 1); the mean and per-variable variances come from 4096 rows of the config's own sampling)")
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--dist", action="store_true",
                   help="multi-GPU: run under `torchrun --nproc-per-node N -m clip_glass_amd.run --dist ...` (one process per GPU, "
                        "RCCL); every rank runs the same seeded search, scores its shard of each population, and one all-gather "
                        "returns all fitness rows; rank 0 writes the outputs")
    return p


def similarity_columns(config):
    """Similarity columns of F for this config: one, or one per entry of a pareto prompt set (the target and config.prompts)."""
    if getattr(config, "prompt_mode", None) == "pareto":
        return 1 + len(getattr(config, "prompts", None) or [])
    return 1


def objective_names(config):
    """Column names of F for this config: similarity (similarity-0 .. similarity-(K - 1) for a pareto prompt set of K entries), then
    discriminator (with D), then lpips (perceptual objective, lambda = 0), then anchor (edit_latent, anchor_lambda = 0)."""
    n = int(config.problem_args["n_obj"])
    K = similarity_columns(config)
    lp_col = getattr(config, "lpips_target", None) is not None and not float(getattr(config, "lpips_lambda", None) or 0.0) > 0.0
    an_col = getattr(config, "edit_latent", None) is not None and not float(getattr(config, "anchor_lambda", None) or 0.0) > 0.0
    sims = ["similarity"] if K == 1 else ["similarity-%d" % t for t in range(K)]
    names = sims + (["discriminator"] if n - K - int(lp_col) - int(an_col) >= 1 else []) + (["lpips"] if lp_col else []) + (["anchor"] if an_col else [])
    return names


def cli_prompts(prompts, image_prompts):
    """config.prompts of the --prompt / --image-prompt flags: the texts first, then the pictures, each as (value, weight)."""
    out = [parse_weighted(t) for t in (prompts or [])]
    for item in (image_prompts or []):
        path, w = parse_weighted(item)
        out.append((("image", path), w))
    return out


def scatter_pairs(names):
    """(i, j, file name) of the Pareto scatters: F.jpg for two objectives (run.py:86-89), one F-<x>-<y>.jpg per pair for three."""
    if len(names) == 2:
        return [(0, 1, "F.jpg")]
    return [(i, j, "F-%s-%s.jpg" % (names[i], names[j])) for i in range(len(names)) for j in range(i + 1, len(names))]


def final_pick_weights(names):
    """Pseudo-weights of the final pick among the Pareto set.  The reference takes (0, 1) on (similarity, discriminator): the most
    realistic point (run.py:103-113).  With the perceptual distance as a third objective the weight is split evenly between realism and
    closeness to the target, (0, .5, .5); without D it goes to the distance, (0, 1).  The latent anchor is one more such column: every
    column that is not a similarity gets the same weight (with D, LPIPS and the anchor a third each).  A default, not a result: the whole
    front is in genetic_result."""
    sims = [n.startswith("similarity") for n in names]
    rest = len(names) - sum(sims)
    if rest == 0:           # nothing but similarities (a pareto prompt set without D or LPIPS): no column is preferred
        return [1.0 / len(names)] * len(names)
    return [0.0 if s else 1.0 / rest for s in sims]


def main(argv=None, extra_config=None):
    config = build_parser().parse_args(argv)
    over = {k: v for k, v in vars(config).items() if v is not None}
    vars(config).update(get_config(config.config))                             # run.py:25
    for k in ("weights", "clip_weights", "clip_model", "clip_resnet", "clip_preprocess", "clip_views", "clip_view_min", "clip_view_flip",
              "clip_view_fixed", "latent_space", "subspace_components", "subspace_layers", "subspace_samples", "subspace_basis", "truncation_psi", "truncation_cutoff", "lpips_target", "lpips_size", "lpips_lambda", "lpips_weights",
              "bpe_path", "pop_size", "stochastic", "target_weight", "prompt_mode", "device_search", "edit_image", "edit_latent", "source_text",
              "anchor_lambda", "edit_sigma", "algorithm", "cma_sigma", "islands", "migrate_every", "migrants"):
        if k in over:
            setattr(config, k, over[k])
    if "prompt" in over or "image_prompt" in over:
        config.prompts = cli_prompts(over.get("prompt"), over.get("image_prompt"))
    if "island_prompt" in over:
        config.island_prompts = list(over["island_prompt"])
    if extra_config:
        vars(config).update(extra_config)
    isl = island_options(config)      # islands where no device search holds them, or own prompts with what they exclude, are refused here
    latent_options(config)      # a latent space / truncation on a BigGAN or GPT2 config is refused here, before anything is loaded
    lpips_options(config)       # ... and so is the perceptual objective on the GPT2 config
    prompt_options(config)      # ... and a prompt set there, or one the engine would refuse
    edit_options(config)        # ... and image editing there, or its anchor on a BigGAN config
    search_options(config)      # ... and what --algorithm cmaes cannot search (several objectives, class bits, tokens, --dist)
    state = dict(iteration=0)
    dist, rank0 = None, True
    if getattr(config, "dist", False):
        import torch
        import torch.distributed as dist
        if not dist.is_initialized():
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            backend = os.environ.get("GLASS_DIST_BACKEND", "nccl")     # "nccl" IS RCCL on ROCm (gloo: CPU tests)
            if backend == "nccl":
                torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
            dist.init_process_group(backend)
        rank0 = dist.get_rank() == 0

    def save_callback(algorithm):                                              # run.py:29-51
        state["iteration"] += 1
        it = state["iteration"]
        if rank0 and (it % config.save_each == 0 or it == config.generations):
            if config.problem_args["n_obj"] == 1:
                X = np.stack([p.X for p in sorted(algorithm.pop, key=lambda p: p.F)])
            else:
                X = np.stack([p.X for p in algorithm.pop])
            ls = config.latent(config)
            ls.set_from_population(X)
            generated = algorithm.problem.generator.generate(ls, minibatch=config.batch_size)
            ext = "txt" if config.task == "img2txt" else "jpg"                   # run.py:46-50
            name = "genetic-it-%d.%s" % (it, ext) if it < config.generations else "genetic-it-final.%s" % ext
            algorithm.problem.generator.save(generated, os.path.join(config.tmp_folder, name))

    problem = GenerationProblem(config, dist=dist)
    config = problem.config     # (the perceptual objective with lambda = 0 searches one more objective: the Generator's copy says so)
    operators = get_operators(config)
    os.makedirs(config.tmp_folder, exist_ok=True)
    if rank0 and getattr(problem.generator, "source_image", None) is not None:      # image editing: what the search moves away from
        problem.generator.save(problem.generator.source_image[None], os.path.join(config.tmp_folder, "source.jpg"))
    # (same seed on every rank => identical GA state everywhere: no broadcast of the population is needed)
    res = search.minimize(problem, config.algorithm, config.pop_size, config.generations, operators["sampling"],
                          seed=config.seed, callback=save_callback, verbose=rank0, mask=operators.get("mask"),
                          device=bool(getattr(config, "device_search", False)),
                          **(dict(islands=isl["islands"], migrate_every=isl["migrate_every"], migrants=isl["migrants"]) if isl else {}),
                          **(dict(cma_sigma=getattr(config, "cma_sigma", None)) if config.algorithm == "cmaes" else {}))
    if not rank0:
        return res
    with open(os.path.join(config.tmp_folder, "genetic_result"), "wb") as f:   # run.py:79-84
        pickle.dump(dict(X=res.X, F=res.F, G=res.G, CV=res.CV,
                         **(dict(islands=[dict(X=r.X, F=r.F, G=r.G, CV=r.CV) for r in res.islands]) if isl else {})), f)
    names = objective_names(config)
    if len(names) >= 2:
        try:                                                                   # run.py:86-89; three objectives: one scatter per pair
            import matplotlib
            matplotlib.use("Agg")
            import matplotlib.pyplot as plt
            Fp = np.atleast_2d(res.F)
            for i, j, fname in scatter_pairs(names):
                plt.figure()
                plt.scatter(Fp[:, i], Fp[:, j], color="red")
                plt.xlabel(names[i]); plt.ylabel(names[j])
                plt.savefig(os.path.join(config.tmp_folder, fname))
                plt.close()
        except Exception as ex:   # plotting is cosmetic
            print("Warning: could not write F.jpg (%s)" % ex)
    if config.problem_args["n_obj"] == 1:
        X = np.stack([p.X for p in sorted(res.pop, key=lambda p: p.F)])
    else:
        X = np.stack([p.X for p in res.pop])
    ls = config.latent(config)
    ls.set_from_population(X)
    saved = ls.state_dict()
    if getattr(problem.generator, "latent_space", None) == "sub":      # next to the coefficients: the dlatents they stand for, which --edit-latent takes
        saved = dict(saved, w_plus=problem.generator.expand_latents(saved["sub"]).reshape(len(saved["sub"]), -1))
    with open(os.path.join(config.tmp_folder, "ls_result"), "wb") as f:        # run.py:101 (same file name, npz payload)
        np.savez(f, **saved)
    if config.problem_args["n_obj"] == 1:
        X = np.atleast_2d(res.X)
    else:
        X = np.atleast_2d(np.atleast_2d(res.X)[search.pseudo_weights_choice(np.atleast_2d(res.F), final_pick_weights(names))])  # run.py:103-113
    ls.set_from_population(X)
    generated = problem.generator.generate(ls)                                 # run.py:118
    ext = "txt" if config.task == "img2txt" else "jpg"                         # run.py:120-125
    problem.generator.save(generated, os.path.join(config.tmp_folder, "output.%s" % ext))
    for i, r in enumerate(res.islands if isl else []):      # every island's own pick, chosen as the overall one is
        if config.problem_args["n_obj"] == 1:
            X = np.atleast_2d(r.X)
        else:
            X = np.atleast_2d(np.atleast_2d(r.X)[search.pseudo_weights_choice(np.atleast_2d(r.F), final_pick_weights(names))])
        ls.set_from_population(X)
        problem.generator.save(problem.generator.generate(ls), os.path.join(config.tmp_folder, "output-island-%d.%s" % (i, ext)))
    return res


if __name__ == "__main__":
    main()
