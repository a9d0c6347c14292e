"""Oracle for the latent spaces and the truncation trick (test infrastructure): the modes of include/glass.h composed from the oracle's own
pieces — oracle.stylegan2_ref.g_mapping, torch.lerp, g_synthesis per minibatch with its noise, then fitness_ref.clip_similarity /
discriminate.  Pinned to the reference's Generator by tests/test_dlatent_ref.py (fixture tests/golden/dlatent_modules.npz)."""
import os

import numpy as np
import torch

from clip_glass_amd import synth
from oracle import fitness_ref, stylegan2_ref as sg

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dlatent_modules.npz")
MINI = dict(channels=[16, 16, 32, 32], latent=32, mapping=2)
SEED = 3                                  # weights (tests/test_oracle_vs_reference.py uses the same mini state)
MODES = {"psi07": (0.7, None), "psi05_cut3": (0.5, 3)}


def n_lat_of(sd):
    b = 0
    while "G_synthesis.conv_blocks.%d.conv_block.0.bias" % b in sd:
        b += 1
    return 2 * b


def layer_psi(n_lat, psi, cutoff):
    """stylegan2/models.py:276-284; None where truncation is off."""
    if psi is None or psi == 1 or cutoff == 0:
        return None
    lp = np.ones(n_lat, np.float32)
    lp[:n_lat if cutoff is None else cutoff] = psi
    return lp


def dlatents(sd, x, space="z", psi=1.0, cutoff=None, avg=None):
    """[P, n_lat, L] float32 tensor: what the synthesis network is fed for rows x of `space` under (psi, cutoff)."""
    n_lat = n_lat_of(sd)
    x = torch.tensor(np.asarray(x).astype(float)).float()               # latent.py:38
    if space == "z":
        d = sg.g_mapping(sd, x)[:, None, :].expand(-1, n_lat, -1)       # models.py:427-430
    elif space == "w":
        d = x[:, None, :].expand(-1, n_lat, -1)
    else:
        d = x.view(x.shape[0], n_lat, -1)
    lp = layer_psi(n_lat, psi, cutoff)
    if lp is not None:                                                  # models.py:323, utils.py:123-125 (fp32: torch.lerp)
        d = torch.lerp(torch.as_tensor(avg).float().expand_as(d), d, torch.tensor(lp).view(1, -1, 1).expand_as(d))
    return d.contiguous()


def synthesize(sd, x, batch_size, noise_fn=None, **mode):
    """Raw generator output [P, 3, R, R], one g_synthesis call per minibatch (models.py:114-116) with its noise planes."""
    d = dlatents(sd, x, **mode)
    assert d.shape[0] % batch_size == 0
    return torch.cat([sg.g_synthesis(sd, d[i * batch_size:(i + 1) * batch_size], noise_fn(i) if noise_fn is not None else None)
                      for i in range(d.shape[0] // batch_size)])


def evaluate(sd, x, text_features, batch_size, use_discriminator, noise_fn=None, clip_size=224, detail=None, **mode):
    """fitness_ref.evaluate with the generator call replaced by `synthesize` in the given mode."""
    with torch.no_grad():
        img = ((synthesize(sd, x, batch_size, noise_fn, **mode) + 1) / 2.0).clip(0, 1)      # utils.py:14-17 biggan_norm
        sim, feats = fitness_ref.clip_similarity(sd, img, text_features, clip_size)
        sim = sim.numpy()
        if detail is not None:
            detail["image"], detail["features"] = img, feats
        if not use_discriminator:
            return -sim
        dis = fitness_ref.discriminate(sd, img, batch_size)
        if detail is not None:
            detail["dis"] = dis
        return np.column_stack((-sim, torch.relu(1 - dis).squeeze(1).numpy()))


# ---- the fixture's inputs (shared by make_dlatent_golden.py, test_dlatent_ref.py and test_gpu_dlatents.py) ----
def fixture_inputs():
    sd = synth.make_state(synth.stylegan2_g_spec(MINI["channels"], MINI["latent"], MINI["mapping"]), SEED)
    z = synth.latents(1, 4, MINI["latent"]).astype(np.float32)
    avg = synth.dlatent_avg(MINI["latent"], SEED)
    planes = synth.g_noise_planes(7, 0, 0, MINI["channels"])
    return sd, z, avg, planes


def fixture_w_plus(w):
    """A w+ population whose eight rows differ: every layer's dlatent is the mapped one moved by its own N(0, 0.3) step."""
    w = np.asarray(w, np.float32)
    return (w[:, None, :] + synth.normal(11, "w_plus", (w.shape[0], 2 * len(MINI["channels"]), w.shape[1]), 0.3)).astype(np.float32)
