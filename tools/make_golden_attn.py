#!/usr/bin/env python3
"""Mint golden cross-attention maps for character localisation.   *** TEST INFRASTRUCTURE ***

The reference computes the head-averaged cross-attention of every decoder pass (`DecoderLayer.forward_stream` returns `ca_weights`,
modules.py:74-79) and `Decoder.forward` discards it.  This script runs the reference's UNMODIFIED `forward` (AR decoding, one refinement
iteration, `max_length` given so that the batch-level early exit never applies) with a forward hook on `decoder.layers[-1].cross_attn`
and keeps the weights of the LAST call — the refinement pass — together with the `tgt_in` that pass ran on (recorded by wrapping the
bound `model.decode`, which the forward calls; the forward's own text is untouched).  Runs in the build container only (needs the
reference checkout), like tools/make_golden_dec_depth.py.

Writes tests/golden/attn_<name>.npz (arrays only: tgt_in, maps, logits) and attn_<name>.json (settings: the weight seed and eos_bias of
oracle/synth.py, the crop seed and indices, so a test regenerates weights and crops).  Crops are chosen so that their strings end strictly
inside the label range at different positions: the padding mask and the zero rows are exercised.

Usage:  python tools/make_golden_attn.py --ref <reference checkout> [--out tests/golden]
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

from oracle.make_golden_train import install_stubs  # noqa: E402
from oracle.synth import CONFIGS, state_dict_fingerprint, synth_images, synth_state_dict  # noqa: E402

# name -> (crops kept, candidates drawn, weight seed, EOS bias of the synthetic head, crop seed)
ATTN_GOLDENS = {
    'parseq-tiny': (2, 32, 0, 2.5, 4321),
    'parseq-patch16-224': (1, 8, 0, 2.5, 4321),
}


@torch.inference_mode()
def run_reference(system, images, max_length):
    """(logits, tgt_in of the last decode call, ca_weights of the last cross-attention call) of the reference's forward."""
    model = system.model
    seen = {}
    hook = model.decoder.layers[-1].cross_attn.register_forward_hook(lambda mod, args, out: seen.__setitem__('weights', out[1].detach().clone()))
    decode = model.decode

    def recording_decode(tgt, *a, **k):
        seen['tgt_in'] = tgt.detach().clone()
        return decode(tgt, *a, **k)
    model.decode = recording_decode
    try:
        logits = system.forward(images, max_length)
    finally:
        hook.remove()
        del model.decode
    return logits, seen['tgt_in'], seen['weights']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', required=True, help='checkout of the reference repository')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    args = ap.parse_args()
    install_stubs()
    sys.path.insert(0, args.ref)
    from strhub.models import utils as ref_utils

    for name, (keep, candidates, seed, eos_bias, crop_seed) in ATTN_GOLDENS.items():
        cfg = CONFIGS[name]
        torch.manual_seed(0)
        system = ref_utils.create_model(name, decode_ar=True, refine_iters=1).eval()
        tok = system.tokenizer
        assert len(tok) == cfg.num_tokens and (tok.eos_id, tok.bos_id, tok.pad_id) == (cfg.eos_id, cfg.bos_id, cfg.pad_id)
        sd = synth_state_dict(cfg, seed, eos_bias=eos_bias)
        res = system.model.load_state_dict(sd, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        npos = cfg.max_label_length + 1
        cand = synth_images(candidates, cfg, seed=crop_seed)
        logits, _, _ = run_reference(system, cand, cfg.max_label_length)
        assert logits.shape[1] == npos                        # max_length given: every step ran, no early exit
        ids = logits.argmax(-1)
        is_eos = ids == tok.eos_id
        first = torch.where(is_eos.any(-1), is_eos.int().argmax(-1), torch.full((candidates,), npos))
        inside = [i for i in range(candidates) if 1 <= int(first[i]) < npos - 1]
        chosen, ends = [], set()
        for i in inside:                                     # distinct end positions first
            if len(chosen) < keep and int(first[i]) not in ends:
                chosen.append(i); ends.add(int(first[i]))
        assert len(chosen) == keep, (name, 'not enough crops whose string ends inside the label range', first.tolist())
        order = sorted(chosen)
        images = cand[torch.tensor(order)].contiguous()
        logits, tgt_in, weights = run_reference(system, images, cfg.max_label_length)
        assert tuple(weights.shape) == (keep, npos, cfg.num_patches) and tuple(tgt_in.shape) == (keep, npos)
        # the definition writes the rows of padded positions (one past the <eos> position on, model.py:163) as zeros; the reference leaves a
        # soft-max there that nothing reads
        weights = weights.masked_fill(((tgt_in == tok.eos_id).int().cumsum(-1) > 0)[:, :, None], 0.0)
        strings, _ = tok.decode(logits.softmax(-1))
        np.savez_compressed(os.path.join(args.out, f'attn_{name}.npz'), tgt_in=tgt_in.to(torch.int32).numpy(), maps=weights.float().numpy(),
                            logits=logits.float().numpy())
        meta = {'model': name, 'seed': seed, 'eos_bias': eos_bias, 'crop_seed': crop_seed, 'candidates': candidates, 'candidate_ids': order,
                'decode_ar': True, 'refine_iters': 1, 'max_length': cfg.max_label_length, 'strings': strings,
                'grid': [cfg.img_size[0] // cfg.patch_size[0], cfg.img_size[1] // cfg.patch_size[1]], 'patch_size': list(cfg.patch_size),
                'sd_fingerprint': state_dict_fingerprint(sd), 'maps_dtype': 'float32', 'rows_past_eos': 'zeroed', 'torch': torch.__version__}
        with open(os.path.join(args.out, f'attn_{name}.json'), 'w') as f:
            json.dump(meta, f, indent=1)
        print(name, 'kept', order, 'strings', strings, 'row sums', float(weights.sum(-1).min()), float(weights.sum(-1).max()))


if __name__ == '__main__':
    main()
