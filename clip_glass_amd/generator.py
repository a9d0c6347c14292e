"""Evaluation façade — mirror of /root/reference/generator.py on top of the HIP engine.

The reference loads CLIP + the GAN, pre-computes the text feature once (generator.py:16-27)
and exposes generate / clip_similarity / discriminate / save.  Here the GAN, the resize and
CLIP live on the device behind ONE call (`evaluate`), so `_evaluate` makes a single trip;
`generate` / `save` serve run.py's callbacks (run.py:45-51,118-125).
"""
import copy
import os

import numpy as np

from . import synth
from .engine import (LATENT_SPACES, PROMPT_MAX, PROMPT_MODES, Engine, clip_geometry_supported, clip_resnet_supported, clip_view_permille,
                     clip_views_supported, clip_views_tower_rows, lpips_n_obj, lpips_supported, prompt_n_obj, subspace_supported)
from .utils import save_grid, save_image

CLIP_VIT_B32 = (768, 12, 12, 32, 224, 512)
# Named image towers: (width, layers, heads, patch, input_res, embed) as clip/model.py:363-399 derives them from the released
# checkpoints, and the text tower that goes with each (the embed dim is shared).  The engine runs any ViT with head dim 64
# (glass_clip_geometry_supported); these are the ones `config.clip_model` / `--clip-model` can name.
CLIP_MODELS = {
    "ViT-B/32": CLIP_VIT_B32,
    "ViT-B/16": (768, 12, 12, 16, 224, 512),
    "ViT-L/14": (1024, 24, 16, 14, 224, 768),
    "ViT-L/14@336": (1024, 24, 16, 14, 336, 768),
}
CLIP_TEXT_MODELS = {
    "ViT-B/32": dict(width=512, layers=12),
    "ViT-B/16": dict(width=512, layers=12),
    "ViT-L/14": dict(width=768, layers=12),
    "ViT-L/14@336": dict(width=768, layers=12),
}
DEFAULT_CLIP_MODEL = "ViT-B/32"
# CLIP's ResNet image towers (clip/model.py:92-149), named on their own (`config.clip_resnet` / `--clip-resnet`): (layers per stage, stem
# width, input_res, embed) as clip/model.py:373-379 derives them from the released checkpoints, and the text tower of each.  The engine
# runs any such tower whose width is a multiple of 64 (glass_clip_resnet_supported): RN50x4 / x16 (widths 80 / 96) are not among them.
CLIP_RESNET_MODELS = {
    "RN50": ((3, 4, 6, 3), 64, 224, 1024),
    "RN101": ((3, 4, 23, 3), 64, 224, 512),
}
CLIP_RESNET_TEXT_MODELS = {
    "RN50": dict(width=512, layers=12),
    "RN101": dict(width=512, layers=12),
}
# How a generated image is prepared for CLIP, `config.clip_preprocess` / `--clip-preprocess` -> (clip_resize, clip_normalize) of
# include/glass.h.  "reference": generator.py:45, a point-sampled bilinear resize and no normalisation — what every parity number of this
# project is quoted for.  "antialias": the same bilinear filter widened to the down-scale, so every input pixel counts.  "clip": the transform
# CLIP was trained with (clip/clip.py:68-74), antialiased bicubic Resize + Normalize — a deliberate departure from the reference.
CLIP_PREPROCESS = {"reference": (0, 0), "antialias": (1, 0), "clip": (2, 1)}
DEFAULT_CLIP_PREPROCESS = "reference"


DEFAULT_LATENT_SPACE = "z"


def latent_options(config):
    """(latent_space, truncation_psi, truncation_cutoff) of a config, defaults ("z", 1.0, None) — the reference's search: z through the raw
    generator.  ValueError with a plain message for an unknown space, and for any non-default value on a config whose generator is not a
    StyleGAN2 (BigGAN has its own `truncation`; GPT2 has no dlatents)."""
    def opt(key, default):       # (a flag the command line left unset arrives as None)
        v = getattr(config, key, None)
        return default if v is None else v
    space = opt("latent_space", DEFAULT_LATENT_SPACE)
    psi = float(opt("truncation_psi", 1.0))
    cutoff = getattr(config, "truncation_cutoff", None)
    cutoff = None if cutoff is None else int(cutoff)
    if space not in LATENT_SPACES:
        raise ValueError("unknown latent_space %r: expected one of %s" % (space, ", ".join(LATENT_SPACES)))
    name = str(getattr(config, "config", ""))
    if (space != DEFAULT_LATENT_SPACE or psi != 1.0 or cutoff is not None) and name.split("_")[0] != "StyleGAN2":
        raise ValueError("latent_space / truncation_psi / truncation_cutoff belong to the StyleGAN2 configs (a mapping network and an "
                         "average dlatent); config %r has neither: leave them unset" % name)
    subspace_options(config)        # the subspace_* keys: refused without latent_space "sub", and on the configs refused above
    return space, psi, cutoff


def subspace_options(config):
    """The options of latent space "sub" (include/glass.h "Subspace latent space"): None unless config.latent_space is "sub", else
    dict(components, layers, samples, basis) from subspace_components (K, default 64, capped at dim_z), subspace_layers (a spec for
    subspace.parse_layer_groups, default: one group of every layer), subspace_samples (rows of z the mapping network is probed with, default
    problem.PROBE_ROWS) and subspace_basis (an npz of subspace.save to use instead of probing).  ValueError by name: a subspace_* key
    without latent_space "sub"; any of it on a BigGAN or GPT2 config; a K or sample count out of range; a basis file whose directions do not
    have the network's dim_z entries."""
    from . import subspace
    vals = {k: getattr(config, k, None) for k in subspace.SUBSPACE_KEYS}
    given = [k for k in subspace.SUBSPACE_KEYS if vals[k] is not None]
    space = getattr(config, "latent_space", None) or DEFAULT_LATENT_SPACE
    name = str(getattr(config, "config", ""))
    if (given or space == "sub") and name.split("_")[0] != "StyleGAN2":
        what = "a BigGAN row is z and class bits" if name.startswith("DeepMindBigGAN") else "the GPT2 config searches token rows"
        raise ValueError("%s: latent space sub is a subspace of a StyleGAN2 generator's W; config %r has none (%s): leave these keys unset"
                         % (", ".join(given or ["latent_space"]), name, what))
    if space != "sub":
        if given:
            raise ValueError("%s set without latent_space 'sub': the subspace keys describe that space alone" % ", ".join(given))
        return None
    K = subspace.components_of(config)
    if K < 1:
        raise ValueError("subspace_components must be at least 1, got %r" % (vals["subspace_components"],))
    N = vals["subspace_samples"]
    if N is not None and vals["subspace_basis"] is None and int(N) < K + 1:
        raise ValueError("subspace_samples=%d rows cannot carry %d principal directions: at least components + 1 are needed" % (int(N), K))
    if vals["subspace_basis"] is not None:
        got = subspace.load(vals["subspace_basis"], latent_size=int(config.dim_z))      # (a file of another network's L is refused here)
        if got["components"].shape[0] < K and vals["subspace_components"] is not None:
            raise ValueError("subspace_basis %r holds %d directions and subspace_components asks for %d"
                             % (str(vals["subspace_basis"]), got["components"].shape[0], K))
    return dict(components=K, layers=vals["subspace_layers"], samples=None if N is None else int(N), basis=vals["subspace_basis"])


# ---- perceptual objective (opt-in, include/glass.h): LPIPS-VGG16 distance of every candidate's image to a target image ----
DEFAULT_LPIPS_SIZE = 256       # what the reference's projector feeds its LPIPS (stylegan2/project.py:107)
LPIPS_KEYS = ("lpips_target", "lpips_size", "lpips_lambda", "lpips_weights")


def lpips_options(config):
    """None while `lpips_target` is unset (the default: today's pass), else dict(target, size, lam, weights) from the config keys
    lpips_target (a path opened with PIL, or an array [3, H, W] in [0, 1]), lpips_size (256), lpips_lambda (0: the distance is one more
    objective; > 0: it is added to the first, times lambda) and lpips_weights (a torch file with the keys of include/glass.h, or
    "synthetic:<seed>").  ValueError, before any weight is looked for, on the GPT2 config (no image is generated there), for the other
    keys without a target, and for a size the library refuses."""
    vals = {k: getattr(config, k, None) for k in LPIPS_KEYS}
    given = [k for k in LPIPS_KEYS if vals[k] is not None]
    if not given:
        return None
    if getattr(config, "task", "txt2img") == "img2txt":
        raise ValueError("%s: the perceptual objective compares generated images with a target image; the img2txt task (config %r) "
                         "generates none: leave the lpips_* keys unset" % (", ".join(given), str(getattr(config, "config", "GPT2"))))
    if vals["lpips_target"] is None:
        raise ValueError("%s set without lpips_target: the perceptual objective is off unless a target image is given" % ", ".join(given))
    size = DEFAULT_LPIPS_SIZE if vals["lpips_size"] is None else int(vals["lpips_size"])
    lam = 0.0 if vals["lpips_lambda"] is None else float(vals["lpips_lambda"])
    if not (lam >= 0.0 and np.isfinite(lam)):
        raise ValueError("lpips_lambda must be finite and >= 0, got %r" % (vals["lpips_lambda"],))
    ok, msg = lpips_supported(0, size)
    if not ok:
        raise ValueError("lpips_size=%d: %s" % (size, msg))
    if vals["lpips_weights"] is None:       # as for CLIP: a silent random-weight VGG16 would steer a whole search by a meaningless distance
        raise RuntimeError("config.lpips_weights is not set: pass the VGG16 + LPIPS linear weights (--lpips-weights PATH), or "
                           "'synthetic:<seed>' explicitly for tests / benchmarks")
    return dict(target=vals["lpips_target"], size=size, lam=lam, weights=str(vals["lpips_weights"]))


def lpips_config(config, opts):
    """The config a search with the perceptual objective runs on: a COPY (the caller's namespace and the config table keep their
    values).  lambda = 0: problem_args["n_obj"] one higher and algorithm "nsga2"; lambda > 0: both as they are."""
    if opts is None or opts["lam"] > 0.0:
        return config
    out = copy.copy(config)
    out.problem_args = dict(config.problem_args, n_obj=int(config.problem_args["n_obj"]) + 1)
    out.algorithm = "nsga2"
    return out


# ---- prompt sets (opt-in, include/glass.h "Prompt sets"): weighted, negative and image prompts; the reference's run.py has one target ----
PROMPT_KEYS = ("prompts", "prompt_mode", "target_weight")
DEFAULT_PROMPT_MODE = "sum"


def parse_weighted(text):
    """"TEXT[::WEIGHT]" of --prompt / --image-prompt -> (TEXT, weight), weight 1 when absent.  The LAST "::" splits, and only where a number
    follows it: a prompt may hold "::" itself."""
    head, sep, tail = str(text).rpartition("::")
    if sep:
        try:
            return head, float(tail)
        except ValueError:
            pass
    return str(text), 1.0


def prompt_options(config):
    """None while `prompts`, `prompt_mode` and `target_weight` are unset (the default: one target through set_target), else
    dict(mode, entries) with entries = [(kind, value, weight), ...]: the config's own target first — ("target", None, target_weight or 1) —
    then config.prompts, a list of (value, weight) pairs whose value is a string (kind "text"), ("image", path_or_array) (kind "image") or a
    float array [clip_embed] (kind "feature").  ValueError with the reason, before any weight is looked for: the GPT2 / img2txt config (its
    cosine is taken on the host, against one image), more than 16 entries, a zero or non-finite weight, an unknown mode, pareto with fewer
    than 2 or more than 4 entries, pareto with lpips_lambda > 0."""
    vals = {k: getattr(config, k, None) for k in PROMPT_KEYS}
    given = [k for k in PROMPT_KEYS if vals[k] is not None]
    if not given:
        return None
    if getattr(config, "task", "txt2img") == "img2txt":
        raise ValueError("%s: prompt sets steer generated images (txt2img); the img2txt task (config %r) compares generated texts with one "
                         "image on the host: leave these keys unset" % (", ".join(given), str(getattr(config, "config", "GPT2"))))
    mode = DEFAULT_PROMPT_MODE if vals["prompt_mode"] is None else vals["prompt_mode"]
    if mode not in PROMPT_MODES:
        raise ValueError("unknown prompt_mode %r: expected one of %s" % (mode, ", ".join(PROMPT_MODES)))
    entries = [("target", None, 1.0 if vals["target_weight"] is None else float(vals["target_weight"]))]
    for i, item in enumerate(vals["prompts"] or []):
        try:
            value, weight = item
        except (TypeError, ValueError):
            raise ValueError("prompts[%d] must be a (value, weight) pair, got %r" % (i, item))
        if isinstance(value, str):
            entries.append(("text", value, float(weight)))
        elif isinstance(value, tuple) and len(value) == 2 and isinstance(value[0], str) and value[0] == "image":
            entries.append(("image", value[1], float(weight)))
        else:
            entries.append(("feature", np.asarray(value, dtype=np.float32).reshape(-1), float(weight)))
    if len(entries) > PROMPT_MAX:
        raise ValueError("a prompt set holds at most %d entries (the target and the prompts), got %d" % (PROMPT_MAX, len(entries)))
    for i, (kind, _, w) in enumerate(entries):
        if not np.isfinite(w) or w == 0.0:
            raise ValueError("prompt weight %d (%s) must be finite and non-zero, got %r: a negative weight steers away from the prompt, "
                             "an entry to ignore is left out" % (i, "target_weight" if kind == "target" else kind, w))
    if mode == "pareto":
        if not 2 <= len(entries) <= 4:
            raise ValueError("prompt_mode 'pareto' gives every entry its own objective: 2 to 4 entries (the target and the prompts), got %d"
                             % len(entries))
        lam = getattr(config, "lpips_lambda", None)
        if getattr(config, "lpips_target", None) is not None and lam is not None and float(lam) > 0.0:
            raise ValueError("prompt_mode 'pareto' with lpips_lambda > 0: lambda folds the distance into THE similarity objective, and a "
                             "pareto set has one per prompt: use lpips_lambda 0 (the distance as an objective of its own)")
    return dict(mode=mode, entries=entries)


def prompt_config(config, opts):
    """The config a pareto prompt set searches: a COPY (as lpips_config's, and applied AFTER it: prompt_config(lpips_config(config, lp),
    opts)) with problem_args["n_obj"] = K + discriminator + (the LPIPS distance as a column) and algorithm "nsga2".  Mode sum, and no set,
    search the config as it is."""
    if opts is None or opts["mode"] != "pareto":
        return config
    lam = getattr(config, "lpips_lambda", None)
    lp_col = getattr(config, "lpips_target", None) is not None and not float(lam or 0.0) > 0.0
    has_d = bool(getattr(config, "use_discriminator", False)) and int(config.problem_args["n_obj"]) - int(lp_col) == 2
    out = copy.copy(config)
    out.problem_args = dict(config.problem_args, n_obj=prompt_n_obj(len(opts["entries"]), has_d, lp_col))
    out.algorithm = "nsga2"
    return out


# ---- image editing (opt-in, include/glass.h "Image editing"): a directional objective relative to a source image, a latent anchor, and a
# search that starts at the source; the reference's run.py has none of it ----
EDIT_KEYS = ("edit_image", "edit_latent", "source_text", "anchor_lambda", "edit_sigma")
# The spread of generation 0 around the source row, in the row's own units: a search setting, not a measurement.  z rows are N(0, 1) and
# dlatents have a spread of the same order, so 0.1 starts every candidate a tenth of a typical coordinate away from the source — close
# enough to be the same face, far enough for crossover to have something to combine.
DEFAULT_EDIT_SIGMA = 0.1


def load_edit_latent(value):
    """config.edit_latent as one float32 row: a path to a .npy, or an array of one row."""
    row = np.load(value) if isinstance(value, (str, os.PathLike)) else np.asarray(value)
    row = np.asarray(row, dtype=np.float32)
    if row.ndim == 2 and row.shape[0] == 1:
        row = row[0]
    if row.ndim != 1 or not np.isfinite(row).all():
        raise ValueError("edit_latent must be ONE finite row of the current latent space, got shape %r" % (row.shape,))
    return np.ascontiguousarray(row)


def edit_options(config):
    """None while every key of EDIT_KEYS is unset (the default: today's search), else dict(image, latent, source_text, lam, sigma, anchor,
    anchor_column): edit_image (a path or an array [3, H, W] in [0, 1]: the source of the directional objective), edit_latent (a path to a
    .npy or an array: one row of the current latent space — the source image is generated from it, the latent anchor is that row, and
    generation 0 starts at it), source_text (what the source shows: required as soon as a source is set), anchor_lambda (0: the anchor is an
    objective of its own; > 0: added to the similarity objective, times lambda) and edit_sigma (the spread of generation 0 around the
    source row, DEFAULT_EDIT_SIGMA).  ValueError by name, before any weight is looked for: the GPT2 / img2txt config refuses every key; the
    BigGAN configs refuse edit_latent and anchor_lambda (no dlatents); a source without source_text; the other keys without a source;
    anchor_lambda or edit_sigma without edit_latent; anchor_lambda > 0 with a pareto prompt set."""
    vals = {k: getattr(config, k, None) for k in EDIT_KEYS}
    given = [k for k in EDIT_KEYS if vals[k] is not None]
    if not given:
        return None
    name = str(getattr(config, "config", ""))
    if getattr(config, "task", "txt2img") == "img2txt":
        raise ValueError("%s: image editing moves generated images away from a source image; the img2txt task (config %r) generates none: "
                         "leave these keys unset" % (", ".join(given), name or "GPT2"))
    if name.split("_")[0] != "StyleGAN2":
        bad = [k for k in ("edit_latent", "anchor_lambda") if vals[k] is not None]
        if bad:
            raise ValueError("%s: the latent anchor is a distance between dlatents of a StyleGAN2 generator; config %r has none (give the "
                             "source as edit_image)" % (", ".join(bad), name))
    if vals["edit_image"] is None and vals["edit_latent"] is None:
        raise ValueError("%s set without a source: give edit_image (a picture) or edit_latent (a latent row)" % ", ".join(given))
    if vals["source_text"] is None or not str(vals["source_text"]).strip():
        raise ValueError("source_text is required with %s: the objective follows the direction from what the source shows to the target"
                         % ("edit_image" if vals["edit_image"] is not None else "edit_latent"))
    for k in ("anchor_lambda", "edit_sigma"):
        if vals[k] is not None and vals["edit_latent"] is None:
            raise ValueError("%s set without edit_latent: the anchor and the start of the search are a latent row" % k)
    lam = 0.0 if vals["anchor_lambda"] is None else float(vals["anchor_lambda"])
    if not (lam >= 0.0 and np.isfinite(lam)):
        raise ValueError("anchor_lambda must be finite and >= 0, got %r" % (vals["anchor_lambda"],))
    sigma = DEFAULT_EDIT_SIGMA if vals["edit_sigma"] is None else float(vals["edit_sigma"])
    if not (sigma > 0.0 and np.isfinite(sigma)):
        raise ValueError("edit_sigma must be finite and > 0, got %r" % (vals["edit_sigma"],))
    if lam > 0.0 and getattr(config, "prompt_mode", None) == "pareto":
        raise ValueError("anchor_lambda > 0 with prompt_mode 'pareto': lambda folds the distance into THE similarity objective, and a pareto "
                         "set has one per prompt: use anchor_lambda 0 (the distance as an objective of its own)")
    anchor = vals["edit_latent"] is not None
    return dict(image=vals["edit_image"], latent=vals["edit_latent"], source_text=str(vals["source_text"]), lam=lam, sigma=sigma, anchor=anchor,
                anchor_column=anchor and lam == 0.0)


def edit_config(config, opts):
    """The config a search with the anchor as its own objective runs on: a COPY (as lpips_config's and prompt_config's, applied AFTER both)
    with problem_args["n_obj"] one higher and algorithm "nsga2".  No anchor, or anchor_lambda > 0: the config as it is."""
    if opts is None or not opts["anchor_column"]:
        return config
    out = copy.copy(config)
    out.problem_args = dict(config.problem_args, n_obj=int(config.problem_args["n_obj"]) + 1)
    out.algorithm = "nsga2"
    return out


def _unit64(v):
    v = np.asarray(v, dtype=np.float64)
    return v / max(float(np.linalg.norm(v)), 1e-8)


def edit_directions(features, kinds, source_text_feature, source_image_feature):
    """The entries of the set as directions (float32 [T, E]): for a text entry (kinds "target", "text", "feature")
    normalise(unit(g_t) - unit(g_source_text)); for an image prompt (kind "image") normalise(unit(g_t) - unit(s_whole_image)).  Computed in
    float64 on the host.  ValueError for an entry that IS its source (a zero direction: nothing to follow)."""
    rows = []
    for t, (f, kind) in enumerate(zip(features, kinds)):
        base = source_image_feature if kind == "image" else source_text_feature
        d = _unit64(f) - _unit64(base)
        n = float(np.linalg.norm(d))
        if not n > 1e-6:
            raise ValueError("prompt %d (%s) is the same as its source (%s): the direction between them is zero" %
                             (t, kind, "the source image" if kind == "image" else "source_text"))
        rows.append(d / n)
    return np.asarray(rows, dtype=np.float32)


def edit_start_population(source_row, n_samples, sigma, xl, xu, normal):
    """Generation 0 of a search that starts at the source: row 0 is the source row itself, rows 1 and up are source + sigma * N(0, 1)
    (normal(size) draws them), everything clipped to [xl, xu] — which problem.edit_bounds has widened to contain the source."""
    src = np.asarray(source_row, dtype=np.float64).reshape(1, -1)
    X = src + float(sigma) * np.asarray(normal((int(n_samples), src.shape[1])), dtype=np.float64)
    X[0] = src[0]
    return np.clip(X, xl, xu)


def prepare_lpips_target(target, size):
    """The target image as the engine takes it: float32 [3, size, size] in [-1, 1].  target: a path (opened with PIL, RGB, / 255), a PIL
    image, or an array [3, H, W] in [0, 1].  Centre-crop to the largest square, then down to `size`: where the square's side is a multiple
    of size, the exact box mean — the area downscale the generated images get (stylegan2/project.py:113-122); otherwise (and when the
    square is smaller than size) PIL's antialiased bicubic resize of the float channels, which is NOT that filter: prefer a target whose
    shorter side is a multiple of size.  Then 2 x - 1."""
    if isinstance(target, (str, os.PathLike)) or hasattr(target, "convert"):
        from PIL import Image
        img = Image.open(target) if not hasattr(target, "convert") else target
        a = np.asarray(img.convert("RGB"), dtype=np.float32).transpose(2, 0, 1) / 255.0
    else:
        a = np.asarray(target, dtype=np.float32)
    if a.ndim != 3 or a.shape[0] != 3:
        raise ValueError("lpips_target must be an image [3, H, W] in [0, 1], got shape %r" % (a.shape,))
    _, H, W = a.shape
    side = min(H, W)
    top, left = (H - side) // 2, (W - side) // 2
    a = a[:, top:top + side, left:left + side]
    if side % size == 0:
        b = side // size
        a = a.reshape(3, size, b, size, b).astype(np.float64).mean(axis=(2, 4))
    else:
        from PIL import Image
        a = np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(ch), mode="F").resize((size, size), Image.BICUBIC)) for ch in a])
    return np.ascontiguousarray(2.0 * a - 1.0, dtype=np.float32)


def load_lpips_state(weights):
    """Engine tensors of the perceptual objective: "synthetic[:seed]" -> synth.lpips_state; otherwise a torch file holding
    "lpips.features.N.{weight,bias}" (torchvision's vgg16 `features` keys; the prefix may be missing) and "lpips.lin.K.weight"."""
    if weights.startswith("synthetic"):
        return synth.lpips_state(int(weights.split(":")[1]) if ":" in weights else 0)
    import torch
    sd = torch.load(weights, map_location="cpu")
    state = {}
    for k, v in sd.items():
        k = k if k.startswith("lpips.") else "lpips." + k
        a = np.asarray(v.float().numpy() if hasattr(v, "float") else v, dtype=np.float32)
        state[k] = a.reshape(-1) if k.startswith("lpips.lin.") else a
    return state


def clip_model_geometry(name):
    """Geometry of a named image tower; ValueError lists the names when it is not one of them."""
    if name not in CLIP_MODELS:
        raise ValueError("unknown CLIP model %r: expected one of %s" % (name, ", ".join(sorted(CLIP_MODELS))))
    return CLIP_MODELS[name]


def clip_model_name(geometry):
    """Name of the tower with this geometry, or None."""
    geometry = tuple(int(v) for v in geometry)
    for name, g in CLIP_MODELS.items():
        if g == geometry:
            return name
    return None


def clip_preprocess_fields(name):
    """(clip_resize, clip_normalize) of a named preprocessing (None: the default); ValueError lists the names otherwise."""
    name = DEFAULT_CLIP_PREPROCESS if name is None else name
    if name not in CLIP_PREPROCESS:
        raise ValueError("unknown clip_preprocess %r: expected one of %s" % (name, ", ".join(CLIP_PREPROCESS)))
    return CLIP_PREPROCESS[name]


def clip_resnet_geometry(name):
    """Geometry of a named ResNet image tower; ValueError lists the names when it is not one of them."""
    if name not in CLIP_RESNET_MODELS:
        raise ValueError("unknown CLIP ResNet model %r: expected one of %s" % (name, ", ".join(sorted(CLIP_RESNET_MODELS))))
    return CLIP_RESNET_MODELS[name]


def clip_resnet_name(geometry):
    """Name of the ResNet tower with this geometry, or None."""
    geometry = normalize_resnet_geometry(geometry)
    for name, g in CLIP_RESNET_MODELS.items():
        if g == geometry:
            return name
    return None


def normalize_resnet_geometry(geometry):
    """(layers4, width, res, embed) as plain ints; ValueError when it is not of that form."""
    try:
        layers, width, res, embed = geometry
        layers = tuple(int(v) for v in layers)
    except (TypeError, ValueError):
        raise ValueError("a CLIP ResNet geometry is (layers4, width, input_res, embed), got %r" % (geometry,))
    if len(layers) != 4:
        raise ValueError("a CLIP ResNet geometry holds four stage depths, got %r" % (layers,))
    return (layers, int(width), int(res), int(embed))


def is_resnet_geometry(geometry):
    """True for a ResNet tower's (layers4, width, res, embed), False for a ViT's six fields."""
    return len(geometry) == 4


def resnet_engine_fields(geometry):
    """The six shared glass_config fields of a ResNet tower: (width, bottlenecks, heads, 32, res, embed) (include/glass.h)."""
    layers, width, res, embed = normalize_resnet_geometry(geometry)
    return (width, sum(layers), width * 32 // 64, 32, res, embed)


def check_clip_geometry(geometry):
    """Raise ValueError with the library's message when the engine cannot run this image tower — before any engine is built."""
    if is_resnet_geometry(geometry):
        ok, msg = clip_resnet_supported(geometry)
        if not ok:
            raise ValueError("CLIP ResNet image tower %s: %s" % (normalize_resnet_geometry(geometry), msg))
        return
    ok, msg = clip_geometry_supported(geometry)
    if not ok:
        raise ValueError("CLIP image tower %s: %s" % (tuple(int(v) for v in geometry), msg))


def clip_geometry_from_state(state):
    """(width, layers, heads, patch, input_res, embed) of the VISUAL tower from a CLIP state dict keyed as
    clip/model.py:363-399 reads it (only `clip.visual.*` blocks count: the text tower has resblocks too)."""
    width = state["clip.visual.conv1.weight"].shape[0]
    patch = state["clip.visual.conv1.weight"].shape[-1]
    grid = round((state["clip.visual.positional_embedding"].shape[0] - 1) ** 0.5)
    layers = len([k for k in state if k.startswith("clip.visual.") and k.endswith(".attn.in_proj_weight")])
    return (width, layers, width // 64, patch, patch * grid, state["clip.visual.proj"].shape[1])


def clip_state_is_resnet(state):
    """A checkpoint decides for itself, as build_model does (clip/model.py:364): no visual.proj means a ModifiedResNet."""
    return "clip.visual.proj" not in state


def clip_resnet_geometry_from_state(state):
    """(layers4, width, input_res, embed) of a ResNet VISUAL tower, read as clip/model.py:373-379 reads it; the embed dim from the
    attention pool's output projection (a visual-only state has no text_projection)."""
    layers = tuple(len(set(k.split(".")[3] for k in state if k.startswith("clip.visual.layer%d." % b))) for b in (1, 2, 3, 4))
    width = state["clip.visual.layer1.0.conv1.weight"].shape[0]
    n_tok = state["clip.visual.attnpool.positional_embedding"].shape[0]
    grid = round((n_tok - 1) ** 0.5)
    if grid * grid + 1 != n_tok:
        raise ValueError("clip.visual.attnpool.positional_embedding has %d rows: not a square grid plus one" % n_tok)
    return (layers, int(width), 32 * grid, int(state["clip.visual.attnpool.c_proj.weight"].shape[0]))


def clip_state_from_checkpoint(sd, with_text):
    """reference CLIP state dict (clip.load(...).state_dict(), clip/clip.py:64-78; keys as build_model reads them,
    clip/model.py:363-399) -> engine tensors under "clip." + key.  The three geometry scalars of the jit archive and
    logit_scale are not weights of either tower."""
    state = {}
    for k, v in sd.items():
        if k in ("input_resolution", "context_length", "vocab_size", "logit_scale"):
            continue
        if k.startswith("visual.") or with_text:
            state["clip." + k] = np.asarray(v.float().numpy() if hasattr(v, "float") else v, dtype=np.float32)
    return state


def _load_clip_state(config, with_text):
    w = getattr(config, "clip_weights", None)
    if w is None:
        # the reference always loads the pretrained ViT-B/32 (clip/clip.py:29-33); a silent random-weight CLIP would run a
        # whole search against meaningless fitness values
        raise RuntimeError("config.clip_weights is not set: pass a CLIP ViT checkpoint (--clip-weights PATH), or "
                           "'synthetic:<seed>' explicitly for tests / benchmarks")
    w = str(w)
    rn_name, rn_geom = getattr(config, "clip_resnet", None), getattr(config, "clip_resnet_geometry", None)
    if (rn_name is not None or rn_geom is not None) and (getattr(config, "clip_model", None) is not None
                                                          or getattr(config, "clip_geometry", None) is not None):
        raise ValueError("clip_model / clip_geometry (a ViT image tower) and clip_resnet / clip_resnet_geometry (a ResNet one) are both "
                         "set: choose one")
    if rn_name is not None:
        clip_resnet_geometry(rn_name)        # an unknown name fails here, whatever the weights are
    if w.startswith("synthetic"):
        seed = int(w.split(":")[1]) if ":" in w else 0
        if rn_name is not None or rn_geom is not None:
            # an explicit clip_resnet_geometry wins over the name, as clip_geometry does for the ViTs
            geom = normalize_resnet_geometry(clip_resnet_geometry(rn_name) if rn_geom is None else rn_geom)
            state = synth.make_state(synth.clip_resnet_spec(*geom), seed)
            if with_text:
                tg = getattr(config, "clip_text_geometry", None) or (CLIP_RESNET_TEXT_MODELS[rn_name] if rn_geom is None
                                                                     else dict(width=512, layers=12))
                state.update(synth.make_state(synth.clip_text_spec(width=tg["width"], layers=tg["layers"],
                                                                   vocab=tg.get("vocab", 49408), out_dim=geom[3]), seed))
            return state, geom
        # an explicit clip_geometry wins; otherwise the named model (default ViT-B/32) gives both towers' geometry
        model = getattr(config, "clip_model", None) or DEFAULT_CLIP_MODEL
        geom = getattr(config, "clip_geometry", None)
        named = geom is None
        geom = tuple(clip_model_geometry(model) if named else geom)
        state = synth.make_state(synth.clip_visual_spec(geom[0], geom[1], geom[3], geom[4], geom[5]), seed)
        if with_text:
            tg = getattr(config, "clip_text_geometry", None) or (CLIP_TEXT_MODELS[model] if named else dict(width=512, layers=12))
            state.update(synth.make_state(synth.clip_text_spec(width=tg["width"], layers=tg["layers"],
                                                               vocab=tg.get("vocab", 49408), out_dim=geom[5]), seed))
        return state, geom
    import torch   # reference: clip.load -> torch.jit.load(archive).state_dict() (clip/clip.py:64-78)
    try:
        sd = torch.jit.load(w, map_location="cpu").state_dict()
    except RuntimeError:
        sd = torch.load(w, map_location="cpu")
    state = clip_state_from_checkpoint(sd, with_text)
    model = getattr(config, "clip_model", None)
    if clip_state_is_resnet(state):      # the checkpoint decides (clip/model.py:364); a name that disagrees is a mistake
        geom = clip_resnet_geometry_from_state(state)
        held = "%s %s" % (clip_resnet_name(geom) or "an unnamed ResNet tower", geom)
        if model is not None:
            raise ValueError("clip_model %r is a ViT %s, but the checkpoint %s holds %s" % (model, clip_model_geometry(model), w, held))
        want = None if rn_name is None and rn_geom is None else normalize_resnet_geometry(
            clip_resnet_geometry(rn_name) if rn_geom is None else rn_geom)
        if want is not None and want != geom:
            raise ValueError("clip_resnet %r is %s, but the checkpoint %s holds %s" % (rn_name or "(geometry)", want, w, held))
        return state, geom
    geom = clip_geometry_from_state(state)
    if rn_name is not None or rn_geom is not None:
        raise ValueError("clip_resnet %r names a ResNet image tower, but the checkpoint %s holds the ViT %s %s"
                         % (rn_name or "(geometry)", w, clip_model_name(geom) or "an unnamed tower", geom))
    if model is not None and clip_model_geometry(model) != geom:      # the checkpoint decides; a name that disagrees is a mistake
        raise ValueError("clip_model %r is %s, but the checkpoint %s holds %s %s"
                         % (model, clip_model_geometry(model), w, clip_model_name(geom) or "an unnamed tower", geom))
    return state, geom


def clip_preprocess(path_or_image, n_px=224):
    """clip/clip.py:68-74: Resize(n_px, BICUBIC) -> CenterCrop -> RGB -> ToTensor -> Normalize.
    torchvision is absent here; restated with PIL (third-party, unpinned)."""
    from PIL import Image
    img = Image.open(path_or_image) if isinstance(path_or_image, str) else path_or_image
    w, h = img.size
    if w <= h:
        nw, nh = n_px, int(n_px * h / w)
    else:
        nw, nh = int(n_px * w / h), n_px
    img = img.resize((nw, nh), Image.BICUBIC)
    left, top = int(round((nw - n_px) / 2.0)), int(round((nh - n_px) / 2.0))
    img = img.crop((left, top, left + n_px, top + n_px)).convert("RGB")
    a = np.asarray(img, dtype=np.float32).transpose(2, 0, 1) / 255.0
    mean = np.array([0.48145466, 0.4578275, 0.40821073], np.float32)[:, None, None]
    std = np.array([0.26862954, 0.26130258, 0.27577711], np.float32)[:, None, None]
    return (a - mean) / std


# ---- search rule (opt-in, include/glass.h "Device search: sep-CMA-ES"): config.algorithm "cmaes" next to the reference's "ga" / "nsga2" ----
def search_options(config):
    """Refuses, by name and before any weight is looked for, what config.algorithm = "cmaes" cannot search — more than one objective, the
    BigGAN configs' class bits, GPT2's tokens, --dist — each with what to use instead; checks config.cma_sigma.  Any other algorithm: nothing."""
    if getattr(config, "algorithm", None) != "cmaes":
        return None
    name = str(getattr(config, "config", ""))
    if getattr(config, "task", None) == "img2txt":
        raise ValueError("algorithm cmaes samples real-valued rows; the GPT2 config searches integer tokens: use ga")
    if name.startswith("DeepMindBigGAN") or getattr(config, "num_classes", None):
        raise ValueError("algorithm cmaes samples real-valued rows; a BigGAN row is [z | boolean class bits] (HUX / bit-flip): use ga")
    if getattr(config, "dist", False):
        raise ValueError("algorithm cmaes: more than one rank (--dist) is not wired to it: run one rank, or ga / nsga2")
    n_obj = int((getattr(config, "problem_args", None) or {}).get("n_obj", 1))
    if n_obj > 1:
        raise ValueError("algorithm cmaes minimises one objective and config %s has %d (the discriminator's hinge is one of its own): use a _nod "
                         "config, or nsga2" % (name, n_obj))
    if getattr(config, "lpips_target", None) is not None and not float(getattr(config, "lpips_lambda", None) or 0.0) > 0.0:
        raise ValueError("algorithm cmaes minimises one objective; lpips_lambda = 0 makes the LPIPS distance a column of its own: fold it in "
                         "with lpips_lambda > 0, or use nsga2")
    if getattr(config, "edit_latent", None) is not None and not float(getattr(config, "anchor_lambda", None) or 0.0) > 0.0:
        raise ValueError("algorithm cmaes minimises one objective; anchor_lambda = 0 makes the latent anchor a column of its own: fold it in "
                         "with anchor_lambda > 0, or use nsga2")
    if getattr(config, "prompt_mode", None) == "pareto":
        raise ValueError("algorithm cmaes minimises one objective; a pareto prompt set has one per prompt: use prompt_mode sum, or nsga2")
    sigma = getattr(config, "cma_sigma", None)
    if sigma is not None and not (np.isfinite(float(sigma)) and float(sigma) > 0.0):
        raise ValueError("cma_sigma must be finite and positive, got %r" % (sigma,))
    return dict(sigma=1.0 if sigma is None else float(sigma))


# ---- island populations (opt-in, include/glass.h "Device search: islands"): several populations in one engine and one pass ----
ISLAND_KEYS = ("islands", "migrate_every", "migrants", "island_prompts")
ISLANDS_MAX = 64


def island_options(config):
    """None while every key of ISLAND_KEYS is unset (the default: one population), else dict(islands, migrate_every, migrants, prompts):
    `islands` populations of pop_size rows each in one engine (island i under seed + i), ring migration of `migrants` rows every
    `migrate_every` generations (0, the default: never), and `island_prompts`: a list of texts (or ready features [clip_embed]) — `target` is
    island 0's prompt and each further entry adds an island that searches it alone.  ValueError by name, before any weight is looked for:
    the GPT2 / img2txt config, --dist, algorithm cmaes, the host search (islands need device_search), an `islands` that disagrees with the
    prompts, and own prompts together with migration, prompt_mode pareto or an edit source."""
    vals = {k: getattr(config, k, None) for k in ISLAND_KEYS}
    given = [k for k in ISLAND_KEYS if vals[k] is not None]
    if not given:
        return None
    prompts = list(vals["island_prompts"] or [])
    K = int(vals["islands"]) if vals["islands"] is not None else 1 + len(prompts)
    if prompts and K != 1 + len(prompts):
        raise ValueError("islands=%d does not agree with island_prompts: target is island 0's prompt and each of the %d island prompts adds an "
                         "island, which makes %d" % (K, len(prompts), 1 + len(prompts)))
    if not 1 <= K <= ISLANDS_MAX:
        raise ValueError("islands must be in [1, %d], got %d" % (ISLANDS_MAX, K))
    M = 0 if vals["migrate_every"] is None else int(vals["migrate_every"])
    n = 1 if vals["migrants"] is None else int(vals["migrants"])
    if M < 0:
        raise ValueError("migrate_every must be >= 0 (0: never), got %d" % M)
    pop = int(getattr(config, "pop_size", 0) or 0)
    if not 1 <= n <= max(pop // 2, 1):
        raise ValueError("migrants must be in [1, pop_size / 2 = %d] (an island's best rows leave and its worst are replaced), got %d" % (pop // 2, n))
    if getattr(config, "task", "txt2img") == "img2txt":
        raise ValueError("%s: islands are populations of the device search, and the GPT2 config searches integer token rows on the host: "
                         "leave these keys unset" % ", ".join(given))
    if getattr(config, "dist", False):
        raise ValueError("%s: islands run on one rank (--dist is not wired to the device search): run one rank" % ", ".join(given))
    if getattr(config, "algorithm", None) == "cmaes":
        raise ValueError("%s: algorithm cmaes keeps one distribution, not populations; islands of distributions are a different feature: use "
                         "ga or nsga2" % ", ".join(given))
    if not getattr(config, "device_search", False):
        raise ValueError("%s: the host search has no islands: set device_search (run.py --device-search)" % ", ".join(given))
    if prompts:
        if M > 0 and K > 1:
            raise ValueError("island_prompts with migrate_every=%d: a migrant's F would be stale under another island's prompt: use "
                             "migrate_every 0" % M)
        if getattr(config, "prompt_mode", None) == "pareto":
            raise ValueError("island_prompts with prompt_mode 'pareto': an island combines the set's entries into one similarity (mode sum), "
                             "and a pareto set has a column per entry")
        if getattr(config, "edit_image", None) is not None or getattr(config, "edit_latent", None) is not None:
            raise ValueError("island_prompts with an edit source: the set's entries are then directions from one source; give the islands one "
                             "target")
    return dict(islands=K, migrate_every=M, migrants=n, prompts=prompts)


def island_config(config, opts):
    """The config an island search with own prompts runs on: a COPY whose prompt set holds the island prompts behind the caller's entries,
    with weight 1 each (the islands' weight table decides which island looks at which)."""
    if opts is None or not opts["prompts"]:
        return config
    out = copy.copy(config)
    out.prompts = list(getattr(config, "prompts", None) or []) + [(p, 1.0) for p in opts["prompts"]]
    return out


def island_weight_table(weights, n_islands):
    """The islands' weights [K, T] over a prompt set whose last K - 1 entries are the island prompts: island 0 keeps the caller's own
    entries (the target and its prompts, with their weights), island i >= 1 a single 1 on its own entry."""
    w = np.asarray(weights, np.float32).reshape(-1)
    K, T = int(n_islands), w.size
    table = np.zeros((K, T), np.float32)
    table[0, :T - (K - 1)] = w[:T - (K - 1)]
    for i in range(1, K):
        table[i, T - K + i] = 1.0
    return table


class Generator:
    def __init__(self, config, dist=None):
        search_options(config)      # algorithm "cmaes": what it cannot search is refused here, before any weight is looked for
        # island populations (opt-in): refused by name here for GPT2, --dist, cmaes and the host search; own prompts join the prompt set
        self.islands = island_options(config)
        config = island_config(config, self.islands)
        # perceptual objective (opt-in): refused for the GPT2 config here, before any weight is looked for; with lambda = 0 the search gets
        # one more objective — on a copy of the config, which callers read back as `generator.config`
        self.lpips = lpips_options(config)
        # prompt set (opt-in): refused for the GPT2 config the same way; a pareto set searches one objective per entry, on a copy too
        self.prompts = prompt_options(config)
        # image editing (opt-in): refused by name for the GPT2 config (every key) and the BigGAN configs (the anchor's keys) here, before any
        # engine is built; the anchor as its own objective searches one more column, on a copy as well
        self.edit = edit_options(config)
        base_n_obj = int((getattr(config, "problem_args", None) or {}).get("n_obj", 1))
        config = edit_config(prompt_config(lpips_config(config, self.lpips), self.prompts), self.edit)
        self.config = config
        self.augmentation = None
        self.model = config.model(config)                                   # generator.py:19
        # dist = None: pick up the process group when one is initialised (a `torchrun` launch: one process per GPU, backend
        # "nccl" = RCCL); every rank then scores its contiguous shard of the SAME population and one all-gather returns all rows
        if dist is None:
            try:
                import torch.distributed as td
                if td.is_available() and td.is_initialized() and td.get_world_size() > 1:
                    dist = td
            except ImportError:
                pass
        sharded = dist is not None and dist.is_initialized() and dist.get_world_size() > 1
        device = getattr(config, "device", 0)
        if sharded and getattr(config, "device_per_rank", None) is None:
            # one process per GPU: every rank sees the same command line ("cuda", "cuda:0", 0 ...), so the device is this rank's
            # LOCAL_RANK unless the caller names a device per rank explicitly (config.device_per_rank = [ids], indexed by rank)
            device = int(os.environ.get("LOCAL_RANK", dist.get_rank()))
        elif sharded:
            device = int(config.device_per_rank[dist.get_rank()])
        elif ":" in str(device):
            device = int(str(device).split(":")[1])
        elif not isinstance(device, int):       # bare "cuda"
            device = 0
        pop = int(getattr(config, "max_pop", max(config.pop_size, config.batch_size) * (self.islands["islands"] if self.islands else 1)))
        self.generation = 0
        self.sharder = None
        self.clip_preprocess = getattr(config, "clip_preprocess", None) or DEFAULT_CLIP_PREPROCESS
        clip_resize, clip_normalize = clip_preprocess_fields(self.clip_preprocess)
        # crop views (opt-in, include/glass.h): a candidate's score is the mean similarity over `clip_views` views of its image
        self.clip_views = int(getattr(config, "clip_views", 0) or 0)
        # latent space / truncation trick (opt-in, include/glass.h); refused here for the BigGAN and GPT2 configs, before anything is loaded
        self.latent_space, self.truncation_psi, self.truncation_cutoff = latent_options(config)
        self.subspace = subspace_options(config)       # latent space "sub" (opt-in): None in every other space
        def view_opt(key, default):      # (a flag the command line left unset arrives as None)
            v = getattr(config, key, None)
            return default if v is None else v
        view_kw = dict(clip_views=self.clip_views, clip_view_min=float(view_opt("clip_view_min", 0.5)),
                       clip_view_flip=bool(view_opt("clip_view_flip", True)),
                       clip_view_fixed=bool(view_opt("clip_view_fixed", False))) if self.clip_views else {}
        # device search (opt-in, include/glass.h "Device search"): the engine keeps the population and runs the generation step; its buffers
        # are sized in finalize, so the engine is told here.  StyleGAN2 rows are real-valued (set_search), BigGAN rows are [z | class bits]
        # (set_search_mixed); the GPT2 config is refused by name: its scoring goes through the host tokenizer every generation
        self.device_search = bool(getattr(config, "device_search", False))
        if self.device_search and config.task == "img2txt":
            raise ValueError("device_search: the GPT2 config searches integer token rows (int_sbx / int_pm): it keeps the host search")
        if sharded and getattr(config, "algorithm", None) == "cmaes":
            raise ValueError("algorithm cmaes: more than one rank (--dist) is not wired to it: run one rank, or ga / nsga2")
        if self.device_search and sharded:
            raise ValueError("device_search: more than one rank (--dist) is not wired to the device search yet: run one rank, or the host search")
        if config.task == "img2txt":                                        # generator.py:25-27, 52-59
            if self.clip_views:
                raise ValueError("clip_views=%d scores crops of generated images (txt2img); the img2txt task has none: leave it at 0"
                                 % self.clip_views)
            if (clip_resize, clip_normalize) != (0, 0):
                # no image is generated here: the target image goes through clip_preprocess() below (clip/clip.py:68-74) either way
                raise ValueError("clip_preprocess=%r applies to generated images (txt2img); the img2txt task has none: leave it at %r"
                                 % (self.clip_preprocess, DEFAULT_CLIP_PREPROCESS))
            clip_state, geom = _load_clip_state(config, True)
            check_clip_geometry(geom)
            tower = self._clip_tower(geom)
            self.engine = Engine([], latent_size=4, mapping_layers=0, batch_size=1, use_discriminator=False, n_obj=1,
                                 max_pop=pop, noise_mode=0, device=device, **tower)
            self.engine.load_state(self.model.state)
            self.engine.load_state(clip_state)
            self.engine.finalize()
            self.model.engine = self.engine
            if getattr(config, "target_features", None) is not None:
                self.image_features = np.asarray(config.target_features, np.float32).reshape(1, -1)
            else:
                self.image_features = self.engine.encode_image(clip_preprocess(config.target, self.clip_geometry[4])[None])
            from .tokenizer import DEFAULT_BPE, ClipTokenizer
            self.tokenizer = ClipTokenizer(getattr(config, "bpe_path", DEFAULT_BPE))
            return
        need_text = getattr(config, "target_features", None) is None or any(
            kind == "text" for kind, _, _ in (self.prompts["entries"] if self.prompts else [])) or (
            self.edit is not None and getattr(config, "source_text_features", None) is None)
        pareto = self.prompts is not None and self.prompts["mode"] == "pareto"
        sim_columns = len(self.prompts["entries"]) if pareto else 0
        clip_state, geom = _load_clip_state(config, need_text)
        check_clip_geometry(geom)        # an unsupported checkpoint fails here, not in generation 1
        tower = self._clip_tower(geom)
        pop = (pop + config.batch_size - 1) // config.batch_size * config.batch_size
        if self.clip_views:                     # refused here with the library's reason, not in the engine's constructor
            tokens, width = clip_views_tower_rows(clip=self.clip_geometry, clip_resnet=self.clip_resnet)
            ok, msg = clip_views_supported(pop, tokens, width, clip_resize, self.clip_views, clip_view_permille(view_kw["clip_view_min"]))
            if not ok:
                raise ValueError("clip_views=%d (clip_preprocess=%r): %s" % (self.clip_views, self.clip_preprocess, msg))
            self.augmentation = dict(kind="crop_views", **view_kw)      # the reference's hook (generator.py:14, 46-47), filled by the engine
        tower.update(view_kw)
        if self.lpips is not None:
            tower.update(lpips_size=self.lpips["size"], lpips_lambda=self.lpips["lam"])
        if pareto:
            tower.update(sim_columns=sim_columns)
        anchor_col = int(self.edit is not None and self.edit["anchor_column"])
        if self.edit is not None and self.edit["anchor"]:
            tower.update(anchor=True, anchor_lambda=self.edit["lam"])
        if hasattr(self.model, "geometry"):     # BigGAN-deep (models.py:64-86)
            self.engine = Engine([], batch_size=config.batch_size, max_pop=pop, chunk=getattr(config, "chunk", 0),
                                 device=device, biggan=self.model.geometry, clip_resize=clip_resize,
                                 clip_normalize=clip_normalize, **tower)
            if self.device_search:
                from .search import DEVICE_PROB_FLIP, DEVICE_PROB_HUX
                try:      # the reference's operators.py:50-58: HUX with probability 0.2 per mating, bit-flip with 10 / 1000 per bit
                    self.engine.set_search_mixed(config.algorithm, int(config.pop_size), int(config.dim_z),
                                                 float(np.float32(config.problem_args["xl"])), float(np.float32(config.problem_args["xu"])),
                                                 prob_x=DEVICE_PROB_HUX, prob_flip=DEVICE_PROB_FLIP, seed=int(getattr(config, "seed", 1) or 1))
                except RuntimeError as ex:
                    self.engine.close()
                    raise ValueError("device_search: %s" % ex)
        else:
            sub_kw = {}
            if self.subspace is not None:       # asked before an engine is built: the library's own rule
                self._plan_subspace(config)
                sub_kw = dict(subspace_shape=self.subspace["shape"])
            self.engine = Engine(self.model.channels[::-1], latent_size=config.dim_z,
                                 mapping_layers=getattr(config, "mapping_layers", 8), batch_size=config.batch_size,
                                 use_discriminator=bool(config.use_discriminator and base_n_obj == 2),
                                 n_obj=(int(config.problem_args["n_obj"]) if pareto          # (the copy's: it counts the anchor's column)
                                        else lpips_n_obj(config.use_discriminator and base_n_obj == 2, self.lpips["lam"]) + anchor_col
                                        if self.lpips is not None else base_n_obj + anchor_col), max_pop=pop, chunk=getattr(config, "chunk", 0),
                                 noise_mode=getattr(config, "noise_mode", 1),
                                 noise_seed=getattr(config, "noise_seed", 0), device=device, clip_resize=clip_resize,
                                 clip_normalize=clip_normalize, latent_space=self.latent_space,
                                 truncation_psi=self.truncation_psi, truncation_cutoff=self.truncation_cutoff, **sub_kw, **tower)
            if self.device_search:
                try:      # bounds: the config's own (z); a search in w / w+ sets its probed bounds after finalize (set_search_operators)
                    self.engine.set_search(config.algorithm, int(config.pop_size), float(np.float32(config.problem_args["xl"])),
                                           float(np.float32(config.problem_args["xu"])), seed=int(getattr(config, "seed", 1) or 1))
                except RuntimeError as ex:
                    self.engine.close()
                    raise ValueError("device_search: %s" % ex)
            if getattr(self.model, "dlatent_avg", None) is not None:
                self.engine.load_state({"dlatent_avg": self.model.dlatent_avg})     # the Generator's own buffer: no sub-model prefix
        if self.islands is not None:
            try:
                self.engine.set_search_islands(self.islands["islands"], self.islands["migrate_every"], self.islands["migrants"])
            except RuntimeError as ex:
                self.engine.close()
                raise ValueError("islands: %s" % ex)
        self.engine.load_state(self.model.state)
        self.engine.load_state(clip_state)
        if self.lpips is not None:
            ok, msg = lpips_supported(self.engine.res, self.lpips["size"])
            if not ok:
                self.engine.close()
                raise ValueError("lpips_size=%d: %s" % (self.lpips["size"], msg))
            self.engine.load_state(load_lpips_state(self.lpips["weights"]))
        self.engine.finalize()
        if self.lpips is not None:
            self.lpips_target = prepare_lpips_target(self.lpips["target"], self.lpips["size"])
            self.engine.set_lpips_target(self.lpips_target)
        if self.latent_space != DEFAULT_LATENT_SPACE:       # the row width of latent.StyleGAN2LatentSpace / operators follows the loaded network
            config.n_lat = self.engine.latent_row()[1]
        if self.subspace is not None:
            self._set_subspace(config)
        texts = [v for kind, v, _ in (self.prompts["entries"] if self.prompts else []) if kind == "text"]
        if getattr(config, "target_features", None) is not None:            # pre-computed text feature
            self.text_features = np.asarray(config.target_features, np.float32).reshape(1, -1)
        else:
            texts = [self.config.target] + texts
        source_feature = getattr(config, "source_text_features", None) if self.edit is not None else None     # pre-computed, as target_features
        if self.edit is not None and source_feature is None:
            texts = texts + [self.edit["source_text"]]                      # the source's text, encoded in the same call, last
        if texts:                                                           # generator.py:23-24; the set's texts in the same call
            from .tokenizer import DEFAULT_BPE, ClipTokenizer
            tok = ClipTokenizer(getattr(config, "bpe_path", DEFAULT_BPE))
            self.tokens = tok.tokenize(texts)
            encoded = self.engine.encode_text(self.tokens)
            if self.edit is not None and source_feature is None:
                source_feature, encoded = encoded[-1], encoded[:-1]
            if getattr(config, "target_features", None) is None:
                self.text_features, encoded = encoded[:1], encoded[1:]
        if self.edit is not None:
            self._set_edit(np.asarray(source_feature, dtype=np.float32).reshape(-1), encoded if texts else None)
        elif self.prompts is None:
            self.engine.set_target(self.text_features[0])
        else:
            self._set_prompts(encoded if texts else None)
        if self.islands is not None and self.islands["prompts"]:      # own prompts: which island looks at which entry of the set
            self.island_weights = island_weight_table(self.prompt_weights, self.islands["islands"])
            self.engine.set_island_weights(self.island_weights)
        if sharded:
            from .parallel import ShardedEvaluator
            self.sharder = ShardedEvaluator(self.engine, dist, dist.get_rank(), dist.get_world_size(), config.batch_size,
                                            device=device)

    def _plan_subspace(self, config):
        """Latent space "sub", before the engine exists: the groups of the style layers (subspace_layers; else the basis file's own; else one
        group of every layer), the number of directions, and the library's verdict on both (subspace_supported) — ValueError with its words."""
        from . import subspace
        sub = self.subspace
        n_lat, L = 2 * len(self.model.channels), int(config.dim_z)
        sub["file"] = subspace.load(sub["basis"], latent_size=L) if sub["basis"] is not None else None
        if sub["layers"] is None and sub["file"] is not None and sub["file"]["layer_group"] is not None:
            lg = np.asarray(sub["file"]["layer_group"], np.int32)
            if lg.shape != (n_lat,):
                raise ValueError("subspace_basis %r: its layer_group holds %d layers and the network has %d: give subspace_layers"
                                 % (str(sub["basis"]), lg.size, n_lat))
        else:
            lg = subspace.parse_layer_groups(sub["layers"], n_lat)
        K = sub["components"]
        if sub["file"] is not None:
            K = min(K, sub["file"]["components"].shape[0])
        G = subspace.n_groups(lg)
        ok, msg = subspace_supported(n_lat, L, G, K, lg)
        if not ok:
            raise ValueError("latent_space 'sub': %s" % msg)
        sub.update(layer_group=lg, shape=(G, K), n_lat=n_lat)

    def _set_subspace(self, config):
        """After finalize: the basis — the file's, or the PCA of the probed mapping network —, the base (the mean dlatent on every layer; with
        edit_latent the file's w or w+ row: the source, whose coefficients are the zero row), into the engine and into subspace.npz."""
        from . import subspace
        sub = self.subspace
        G, K = sub["shape"]
        if sub["file"] is not None:
            mean, comp, std = sub["file"]["mean"], sub["file"]["components"][:K], sub["file"]["stdev"][:K]
        else:
            mean, comp, std = subspace.build(self, config)
        base = None
        if self.edit is not None and self.edit["latent"] is not None:
            base = load_edit_latent(self.edit["latent"])
            L = int(config.dim_z)
            if base.size not in (L, sub["n_lat"] * L):
                raise ValueError("edit_latent holds %d floats; with latent_space 'sub' it is the base of the subspace: a w row (%d floats) or a "
                                 "w+ row (%d floats)" % (base.size, L, sub["n_lat"] * L))
        basis, base = subspace.operands(mean, comp, std, sub["n_lat"], base)
        self.engine.set_subspace(sub["layer_group"], basis, base)
        sub.update(mean=mean, components=comp, stdev=std, basis=basis, base=base)
        config.subspace_shape = (G, K)        # the row width of latent.StyleGAN2LatentSpace / operators follows it
        folder = getattr(config, "tmp_folder", None)
        if folder is not None and int(os.environ.get("RANK", "0")) == 0:      # (under --dist every rank computes the same basis: rank 0 writes it)
            os.makedirs(folder, exist_ok=True)
            subspace.save(os.path.join(folder, "subspace.npz"), mean, comp, std, sub["layer_group"])

    def expand_latents(self, rows):
        """rows of this Generator's latent space -> the dlatents the pass makes its styles from, [N, n_lat, L], in slices of the engine's
        capacity.  Flattened, a result is a w+ row (what edit_latent takes)."""
        x = np.asarray(rows, dtype=np.float32)
        cap = int(self.engine.cfg.max_pop)
        return np.concatenate([self.engine.expand_latents(x[i:i + cap]) for i in range(0, x.shape[0], cap)])

    def _set_prompts(self, text_features):
        """Build the set's features [T, E] in the order of prompt_options' entries and hand it to the engine.  text_features: the encoded
        "text" entries, in order.  An image goes through prepare_lpips_target (centre crop, resize to the generator's side, [-1, 1]) and
        the engine's encode_generated: the feature a generated image with those pixels would get."""
        self._prompt_rows(self.prompts["entries"], text_features)
        self.prompt_mode = self.prompts["mode"]
        self.engine.set_targets(self.prompt_features, self.prompt_weights, self.prompt_mode)

    def _prompt_rows(self, entries, text_features):
        """prompt_features [T, E] and prompt_weights [T] of `entries`, in their order (see _set_prompts)."""
        E = int(self.engine.cfg.clip_embed)
        rows, n_text = [], 0
        for kind, value, _ in entries:
            if kind == "target":
                f = self.text_features[0]
            elif kind == "text":
                f, n_text = text_features[n_text], n_text + 1
            elif kind == "image":
                f = self.engine.encode_generated(prepare_lpips_target(value, self.engine.res)[None])[0]
            else:
                f = value
            f = np.asarray(f, dtype=np.float32).reshape(-1)
            if f.size != E:
                raise ValueError("a prompt feature must hold clip_embed = %d floats, got %d" % (E, f.size))
            rows.append(f)
        self.prompt_features = np.stack(rows)
        self.prompt_weights = np.asarray([w for _, _, w in entries], dtype=np.float32)

    def _set_edit(self, source_text_feature, text_features):
        """Image editing: the source image (edit_image, or the image generated from edit_latent) becomes the engine's direction source, the
        entries of the set — the single target is a set of one — become directions away from the source's text (an image prompt: away from
        the source image's own whole-image feature), and edit_latent's row becomes the latent anchor."""
        ed = self.edit
        if ed["latent"] is not None and self.latent_space == "sub":
            self.edit_row = np.zeros(self.latent_width(), np.float32)      # the file's row is the subspace's base: the source is the zero row
        elif ed["latent"] is not None:
            self.edit_row = load_edit_latent(ed["latent"])
            width = self.latent_width()
            if self.edit_row.size != width:
                raise ValueError("edit_latent holds %d floats; a row of latent space %r has %d" % (self.edit_row.size, self.latent_space, width))
        if ed["image"] is not None:
            source = prepare_lpips_target(ed["image"], self.engine.res)          # centre crop, resize to the generator's side, [-1, 1]
            self.source_image = np.ascontiguousarray((source + 1.0) / 2.0, dtype=np.float32)
        else:       # the row's own picture: generation 0, minibatch 0, first image of a minibatch of copies (that fixes its noise planes)
            tiled = np.tile(self.edit_row[None], (int(self.config.batch_size), 1))
            self.source_image = self.engine.generate(tiled, generation=0, first_minibatch=0)[0]
            source = np.ascontiguousarray(2.0 * self.source_image - 1.0, dtype=np.float32)
        self.source_feature = self.engine.encode_generated(source[None])[0]
        entries = self.prompts["entries"] if self.prompts is not None else [("target", None, 1.0)]
        self._prompt_rows(entries, text_features)
        self.prompt_mode = self.prompts["mode"] if self.prompts is not None else DEFAULT_PROMPT_MODE
        self.source_text_feature = source_text_feature
        self.prompt_directions = edit_directions(self.prompt_features, [k for k, _, _ in entries], source_text_feature, self.source_feature)
        self.engine.set_targets(self.prompt_directions, self.prompt_weights, self.prompt_mode)
        self.engine.set_direction_source(source)
        if ed["anchor"]:
            self.engine.set_anchor(self.edit_row)

    def map_latents(self, z):
        """z [N, dim_z] -> untruncated dlatents w [N, dim_z] through the engine's mapping network, in slices of its capacity."""
        z = np.asarray(z, dtype=np.float32)
        cap = int(self.engine.cfg.max_pop)
        return np.concatenate([self.engine.map_latents(z[i:i + cap]) for i in range(0, z.shape[0], cap)]) if z.shape[0] else z

    def latent_width(self):
        """Floats per population row in this Generator's latent space."""
        return self.engine.latent_row()[0]

    def _clip_tower(self, geom):
        """Record the chosen image tower (clip_geometry: the engine's six shared fields; clip_resnet: the ResNet tuple or None) and
        return the Engine keywords that select it."""
        if is_resnet_geometry(geom):
            self.clip_resnet = normalize_resnet_geometry(geom)
            self.clip_geometry = resnet_engine_fields(geom)
            return dict(clip_resnet=self.clip_resnet)
        self.clip_resnet = None
        self.clip_geometry = tuple(int(v) for v in geom)
        return dict(clip=self.clip_geometry)

    def clip_similarity_texts(self, texts):
        """generator.py:52-59 (img2txt branch): tokenize -> encode_text -> cosine vs the target image feature;
        a tokenisation failure zeroes the WHOLE population, as the reference's bare except does."""
        try:
            tokens = self.tokenizer.tokenize(texts)
        except Exception:
            return np.zeros(len(texts), np.float32)
        tf = self.engine.encode_text(tokens).astype(np.float64)
        im = self.image_features.astype(np.float64)
        den = np.maximum(np.linalg.norm(tf, axis=1) * np.linalg.norm(im, axis=1), 1e-8)
        return ((tf @ im.T)[:, 0] / den).astype(np.float32)

    # --- the hot path: generate + clip_similarity + discriminate in ONE device pass -------------
    def evaluate(self, ls, noise=None, first_minibatch=0):
        if self.config.task == "img2txt":           # problem.py:19-20,27 with the GPT2 config
            # (config.stochastic: each generation draws fresh texts; greedy decoding ignores the generation)
            texts = self.model.generate(*ls(), generation=self.generation, purpose=synth.GPT2_SAMPLE_EVALUATE)
            self.last_texts = texts
            self.generation += 1
            return -self.clip_similarity_texts(texts)[:, None]
        z = ls.population()
        if self.sharder is not None:        # one process per GPU: this rank scores its shard, ONE all-gather of the rows
            if noise is not None or first_minibatch:
                # caller-provided planes / offsets address ONE engine's minibatches; the sharded path derives both from the
                # global minibatch index (device noise), so accepting them here would silently ignore them
                raise ValueError("noise / first_minibatch cannot be combined with a sharded (multi-GPU) Generator")
            F = self.sharder.evaluate_global(z, generation=self.generation)
        else:
            F = self.engine.evaluate(z, generation=self.generation, first_minibatch=first_minibatch, noise=noise)
        self.generation += 1
        return F

    def generate(self, ls, minibatch=None, noise=None):
        """generator.py:29-34 — images [P,3,R,R] float32 after config.norm (biggan_norm); texts for img2txt."""
        if self.config.task == "img2txt":        # deterministic per generation, never the draw evaluate() used
            return self.model.generate(*ls(), generation=self.generation, purpose=synth.GPT2_SAMPLE_SAVE)
        z = ls.population()
        bs = self.config.batch_size
        P = z.shape[0]
        if minibatch is None:                       # run.py:118: whole input as ONE G call
            pad = (-P) % bs
        else:
            assert z.shape[0] % minibatch == 0      # models.py:112
            pad = 0
        if pad:
            z = np.concatenate([z, np.repeat(z[-1:], pad, axis=0)])
        img = self.engine.generate(z, generation=self.generation, noise=noise)[:P]
        return img

    def has_discriminator(self):
        return self.model.has_discriminator()

    def save(self, input, path):
        """generator.py:63-72"""
        if self.config.task == "img2txt":
            with open(path, "w") as f:
                f.write("\n".join(input))
            return
        if input.shape[0] > 1:
            save_grid(input, path)
        else:
            save_image(input[0], path)
