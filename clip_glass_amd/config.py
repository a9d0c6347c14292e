"""Config table — mirror of /root/reference/config.py (same keys and values for the
StyleGAN2 configs; `latent` / `model` point at this package's classes).

Optional keys the table leaves unset (run.py copies them in from its flags): `clip_model` (generator.CLIP_MODELS, default ViT-B/32),
`clip_resnet` (generator.CLIP_RESNET_MODELS: RN50 / RN101 instead of a ViT; `clip_resnet_geometry` = (layers4, width, res, embed) wins over the name) and
`clip_preprocess` — "reference" (default: the reference's resize, generator.py:45), "antialias" or "clip" (generator.CLIP_PREPROCESS);
`clip_views` (0, the default: one whole-image score as the reference computes it; N >= 1: the mean similarity over N crop views of each
image, include/glass.h), with `clip_view_min` (smallest crop side as a fraction of the image side, 0.5), `clip_view_flip` (mirror crops at
random, True) and `clip_view_fixed` (the same crops in every generation, False);
`latent_space` ("z", the default: the reference's search; "w": rows are dlatents, the mapping network is skipped; "w+": one dlatent per
style layer), `truncation_psi` (1.0: off) and `truncation_cutoff` (None: every layer) — the StyleGAN2 configs only (include/glass.h);
refused for the BigGAN and GPT2 configs;
`latent_space` "sub" (rows are coefficients of principal directions of W per group of style layers, include/glass.h "Subspace latent
space") with `subspace_components` (64: directions per group, capped at `dim_z`), `subspace_layers` (unset: one group of every layer; a
spec like "0-3,4-7,8-17": one group per inclusive range, layers not named frozen), `subspace_samples` (4096: rows of z the mapping network
is probed with for the PCA) and `subspace_basis` (an npz with mean, components, stdev[, layer_group] to use instead of probing: the
subspace.npz of an earlier run, or a GANSpace export) — the StyleGAN2 configs only; the `subspace_*` keys are refused without the space,
and all of it for the BigGAN and GPT2 configs.  The bounds stay the config's own (+-10): the coefficients are unit-variance, as z's variables;
`lpips_target` (unset, the default: off; a path or an array [3, H, W] in [0, 1]: the LPIPS-VGG16 distance to that image becomes a search
objective, include/glass.h), with `lpips_size` (256), `lpips_lambda` (0: an objective of its own — the Generator then searches a copy of the
config with `n_obj` one higher and `algorithm` "nsga2", this table is not touched; > 0: added to the similarity objective) and
`lpips_weights` (a torch file or "synthetic:<seed>") — the StyleGAN2 and BigGAN configs; refused for GPT2;
`prompts` (unset, the default: the one `target`; a list of (value, weight) pairs — value a text, ("image", path_or_array) or a ready feature
[clip_embed]; a negative weight steers away from the prompt, include/glass.h "Prompt sets"), with `target_weight` (1: the weight of `target`,
which is always the set's first entry) and `prompt_mode` ("sum", the default: the entries blend into the one similarity objective,
sum_t w_t sim_t / sum_t |w_t|; "pareto": one objective per entry, 2 to 4 — the Generator then searches a copy of the config with `n_obj` =
entries + discriminator + LPIPS column and `algorithm` "nsga2") — the StyleGAN2 and BigGAN configs; refused for GPT2;
`device_search` (False, the default: search.py's host operators; True: the population stays on the GPU and the generation step — tournament,
SBX, polynomial mutation, duplicate flags, survival — runs there, include/glass.h "Device search") — the StyleGAN2 configs and, with
half-uniform crossover (probability 0.2 per mating) and bit-flip (10 / 1000 per bit) on the class bits behind the `dim_z` real columns
("Mixed rows" there), the BigGAN configs, on one rank; refused for the GPT2 config (integer rows, scored through the host tokenizer every
generation: a device step would not remove the round trip) and with `--dist`;
`edit_image` (unset, the default: off; a path or an array [3, H, W] in [0, 1], centre-cropped and resized to the generator's side as an image
prompt is: the similarity becomes directional — how the generated image moved away from this source against how the target moved away
from `source_text`, include/glass.h "Image editing"), `edit_latent` (a path to a .npy, or an array, of one row in the current latent space:
the source image is generated from it, the row is the latent anchor — the mean squared distance between a candidate's dlatents and the
row's — and generation 0 starts at it), `source_text` (what the source shows: required as soon as a source is set), `anchor_lambda` (0:
the anchor distance is an objective of its own — the Generator then searches a copy of the config with `n_obj` one higher and `algorithm`
"nsga2"; > 0: added to the similarity objective) and `edit_sigma` (0.1: the spread of generation 0 around the source row; row 0 is the
source itself) — `edit_image` with the StyleGAN2 and BigGAN configs, `edit_latent` / `anchor_lambda` with the StyleGAN2 configs only; every
key is refused for GPT2;
`algorithm` "cmaes" (instead of the table's "ga": separable CMA-ES, include/glass.h "Device search: sep-CMA-ES" — one objective and
real-valued rows, so the StyleGAN2 `_nod` configs, with `lpips_lambda` / `anchor_lambda` > 0 where those objectives are on; on the host, or
on the GPU with `device_search`) and `cma_sigma` (1.0: the initial step size; the initial mean and variances come from 4096 rows of the
config's own sampling) — refused by name for a config with more than one objective, the BigGAN configs, GPT2 and `--dist`;
`islands` (unset, the default: one population; K: with `device_search`, K populations of `pop_size` rows each — `pop_size` stays the
per-island size, the engine is built for K pop_size rows — in one engine and one pass per generation, island i under seed + i,
include/glass.h "Device search: islands"), with `migrate_every` (0: never; M: every M generations the best rows of island i - 1 replace the
worst of island i), `migrants` (1: rows per migration, at most pop_size / 2) and `island_prompts` (a list of texts or ready features:
`target` is island 0's prompt and each entry adds an island that searches it alone — not with migration, `prompt_mode` "pareto" or an edit
source) — the StyleGAN2 and BigGAN configs with "ga" / "nsga2" on one rank; refused by name for GPT2, `--dist`, "cmaes" and the host search."""
from .latent import DeepMindBigGANLatentSpace, GPT2LatentSpace, StyleGAN2LatentSpace
from .models import GPT2, DeepMindBigGAN, StyleGAN2
from .utils import biggan_denorm, biggan_norm


def _sg2(weights, use_d):
    return dict(
        task="txt2img", dim_z=512, latent=StyleGAN2LatentSpace, model=StyleGAN2, use_discriminator=use_d,
        weights=weights, algorithm="nsga2" if use_d else "ga", norm=biggan_norm, denorm=biggan_denorm,
        pop_size=16, batch_size=4,
        problem_args=dict(n_var=512, n_obj=2 if use_d else 1, n_constr=512, xl=-10, xu=10))


configs = dict(
    GPT2=dict(task="img2txt", dim_z=20, max_tokens_len=30, max_text_len=50, encoder_size=50257,
              latent=GPT2LatentSpace, model=GPT2, use_discriminator=False, init_text="the picture of",
              weights="./gpt2/weights/gpt2-pytorch_model.bin", encoder="./gpt2/weights/encoder.json",
              vocab="./gpt2/weights/vocab.bpe", stochastic=False, algorithm="ga", pop_size=100, batch_size=25,
              problem_args=dict(n_var=20, n_obj=1, n_constr=20, xl=0, xu=50256)),
    DeepMindBigGAN256=dict(task="txt2img", dim_z=128, num_classes=1000, latent=DeepMindBigGANLatentSpace,
                           model=DeepMindBigGAN, weights="biggan-deep-256", use_discriminator=False, algorithm="ga",
                           norm=biggan_norm, denorm=biggan_denorm, truncation=1.0, pop_size=64, batch_size=32,
                           problem_args=dict(n_var=128 + 1000, n_obj=1, n_constr=128, xl=-2, xu=2)),
    DeepMindBigGAN512=dict(task="txt2img", dim_z=128, num_classes=1000, latent=DeepMindBigGANLatentSpace,
                           model=DeepMindBigGAN, weights="biggan-deep-512", use_discriminator=False, algorithm="ga",
                           norm=biggan_norm, denorm=biggan_denorm, truncation=1.0, pop_size=32, batch_size=8,
                           problem_args=dict(n_var=128 + 1000, n_obj=1, n_constr=128, xl=-2, xu=2)),
    StyleGAN2_ffhq_d=_sg2("./stylegan2/weights/ffhq-config-f", True),
    StyleGAN2_car_d=_sg2("./stylegan2/weights/car-config-f", True),
    StyleGAN2_church_d=_sg2("./stylegan2/weights/church-config-f", True),
    StyleGAN2_ffhq_nod=_sg2("./stylegan2/weights/ffhq-config-f", False),
    StyleGAN2_car_nod=_sg2("./stylegan2/weights/car-config-f", False),
    StyleGAN2_church_nod=_sg2("./stylegan2/weights/church-config-f", False),
)


def get_config(name):
    return configs[name]
