#!/usr/bin/env python3
"""Mint training-step golden vectors for encoders of more than 128 tokens.   *** TEST INFRASTRUCTURE ***

ViTSTR (129 tokens: the class token + 128 patches) and PARSeq-patch16-224 (14 x 14 = 196 tokens) train through the key-streaming
encoder attention (parseq_amd/csrc/train_attn_wide.h).  This script runs ONE `training_step` + `loss.backward()` of the reference's
own systems, as oracle/make_golden_train.py does for PARSeq-S, whose helpers (install_stubs, build_system, checksum) it imports
unchanged:
  * the reference's ViTSTR system (strhub/models/vitstr/system.py, configs/model/vitstr.yaml + experiment/vitstr.yaml) on the
    synthetic weights of oracle/vitstr_oracle.py and crops with labels of different lengths;
  * the reference's PARSeq system with the patch16-224 configuration (configs/experiment/parseq-patch16-224.yaml) in evaluation
    mode, the permutations it drew recorded.
Runs in the build container only (needs the reference checkout).

Writes
  tests/golden/vitstr_train.{safetensors,json}        the loss, whole gradients of the small tensors, the L2 norm and a checksum of
                                                      every gradient, the crops' seed and checksum
  tests/golden/parseq-patch16-224_train.safetensors   the permutations drawn, the loss, and whole gradients of the
  tests/golden/parseq-patch16-224_train.json          small tensors; the L2 norm and a checksum of every gradient, the crops'
                                                      seed and checksum (they are regenerated, not stored)

Usage:  python tools/make_golden_train_wide.py --ref <reference checkout> [--out tests/golden]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import vitstr_oracle as V  # noqa: E402
from oracle.make_golden import CHARSET_94  # noqa: E402
from oracle.make_golden_train import build_system, checksum, install_stubs  # noqa: E402
from oracle.synth import CONFIGS, synth_images, synth_state_dict  # noqa: E402

LABELS = ['Hello', 'MI355X', 'x7', 'W0rld#42']
FULL_GRADS = ['head.bias', 'pos_queries', 'decoder.norm.weight', 'decoder.layers.0.self_attn.in_proj_bias',
              'encoder.norm.weight', 'encoder.blocks.0.attn.qkv.bias', 'encoder.blocks.11.attn.qkv.bias',
              'encoder.blocks.11.mlp.fc2.bias', 'encoder.patch_embed.proj.bias']
NP_SEED, TORCH_SEED, IMAGE_SEED = 11, 22, 4321
VITSTR_LABELS = ['Hello', 'a', 'MI355X', 'parallel-decoding', 'x7', 'Permuted_AR_Sequence(25)!', 'stop', 'W0rld#42']
VITSTR_FULL_GRADS = ['head.bias', 'head.weight', 'cls_token', 'pos_embed', 'norm.weight', 'norm.bias', 'blocks.0.attn.qkv.bias',
                     'blocks.11.mlp.fc2.bias', 'patch_embed.proj.bias']
VITSTR_IMAGE_SEED = 2468


def _record(system, loss, full, extra):
    out = {'loss': loss.detach().reshape(1)}
    grads = {}
    for k, p in system.model.named_parameters():
        g = p.grad if p.grad is not None else torch.zeros_like(p)
        grads[k] = {'norm': float(g.double().norm()), 'checksum': checksum(g), 'none': p.grad is None}
        if k in full:
            out['grad.' + k] = g.detach().contiguous()
    meta = dict(extra, loss=float(loss.detach()), grads=grads, torch=torch.__version__)
    return out, meta


def mint_vitstr(ref, out_dir):
    from safetensors.torch import save_file
    install_stubs()
    if ref not in sys.path:
        sys.path.insert(0, ref)
    from strhub.models.vitstr.system import ViTSTR
    # base.py:194-204 reads `self.device` (a LightningModule property; install_stubs' stand-in keeps `_device`)
    ViTSTR.device = property(lambda self: self._device)
    cfg = V.vitstr_config()
    # configs/model/vitstr.yaml: embed_dim 384, num_heads 6; experiment/vitstr.yaml: 32 x 128 crops, 4 x 8 patches; main.yaml: 25 chars
    system = ViTSTR(CHARSET_94, CHARSET_94, cfg.max_label_length, 384, 8.9e-4, 0.075, 0.0, list(cfg.img_size), list(cfg.patch_size),
                    cfg.embed_dim, cfg.enc_num_heads)
    res = system.model.load_state_dict(V.synth_state_dict(cfg, 0), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    images = synth_images(len(VITSTR_LABELS), cfg, seed=VITSTR_IMAGE_SEED)
    loss = system.training_step((images, VITSTR_LABELS), 0)
    loss.backward()
    out, meta = _record(system, loss, VITSTR_FULL_GRADS, {'labels': VITSTR_LABELS, 'image_seed': VITSTR_IMAGE_SEED,
                                                           'image_checksum': checksum(images)})
    save_file(out, os.path.join(out_dir, 'vitstr_train.safetensors'))
    with open(os.path.join(out_dir, 'vitstr_train.json'), 'w') as f:
        json.dump(meta, f, indent=1)
    print('vitstr loss', meta['loss'], 'grad keys', len(meta['grads']))


def mint_parseq_patch16(ref, out_dir):
    from safetensors.torch import save_file
    name = 'parseq-patch16-224'
    cfg = CONFIGS[name]
    system = build_system(ref, cfg).eval()          # .eval(): dropout off, the only non-reproducible part of the step
    system.model.load_state_dict(synth_state_dict(cfg, seed=0), strict=True)
    images = synth_images(len(LABELS), cfg, seed=IMAGE_SEED)
    system.rng = np.random.default_rng(NP_SEED)
    torch.manual_seed(TORCH_SEED)
    drawn = []
    gen = system.gen_tgt_perms
    system.gen_tgt_perms = lambda tgt: drawn.append(gen(tgt)) or drawn[-1]
    loss = system.training_step((images, LABELS), 0)
    loss.backward()
    # the crops are not stored (2.4 MB at 224 x 224): a test regenerates them with synth_images(len(LABELS), cfg, IMAGE_SEED) and checks
    # them against the recorded checksum
    out = {'perms': drawn[0].to(torch.int32), 'loss': loss.detach().reshape(1)}
    grads = {}
    for k, p in system.model.named_parameters():
        g = p.grad if p.grad is not None else torch.zeros_like(p)
        grads[k] = {'norm': float(g.double().norm()), 'checksum': checksum(g), 'none': p.grad is None}
        if k in FULL_GRADS:
            out['grad.' + k] = g.detach().contiguous()
    save_file(out, os.path.join(out_dir, f'{name}_train.safetensors'))
    with open(os.path.join(out_dir, f'{name}_train.json'), 'w') as f:
        json.dump({'labels': LABELS, 'loss': float(loss.detach()), 'np_seed': NP_SEED, 'torch_seed': TORCH_SEED, 'image_seed': IMAGE_SEED,
                   'image_checksum': checksum(images), 'perms': drawn[0].tolist(), 'grads': grads, 'torch': torch.__version__}, f, indent=1)
    print(name, 'loss', float(loss.detach()), 'perms', tuple(drawn[0].shape), 'grad keys', len(grads))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', required=True, help='checkout of the reference repository')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    args = ap.parse_args()
    mint_vitstr(args.ref, args.out)
    mint_parseq_patch16(args.ref, args.out)


if __name__ == '__main__':
    main()
