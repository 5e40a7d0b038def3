#!/usr/bin/env python3
"""Mint golden vectors for PARSeq decoders deeper than one layer (`dec_depth` > 1).   *** TEST INFRASTRUCTURE ***

The reference accepts any decoder depth through its hub keyword arguments (`create_model('parseq', dec_depth=2)`:
configs/model/parseq.yaml exposes `dec_depth`, `Decoder` clones that many layers, modules.py:101-125).  The oracle restatement
under oracle/ is a depth-1 decoder, so every depth > 1 vector here comes from the reference itself.  Runs in the build container
only (needs the reference checkout), like oracle/make_golden_hub.py, whose helpers it imports unchanged.

For every entry of DEC_DEPTH_VARIANTS it
  1. builds the system through the reference's UNMODIFIED `create_model(experiment, **kwargs)` and records the resolved
     configuration and the state_dict key order;
  2. loads the synthetic weights `synth_state_dict(cfg, seed, eos_bias)` with strict=True (seed, eos_bias and the fingerprint are
     recorded, so a test regenerates the weights);
  3. keeps crops whose AR string ends strictly inside the label range at different positions, so that the batch-level early exit
     fires after a mixed batch (model.py:144-145);
  4. runs the seven modes of make_golden_hub.modes_for plus 'ar1_full' (AR + 1 refinement with max_length given) through the
     system's forward.  In the testing-mode refinement modes (ar1, ar2) the reference's forward RAISES once the early exit fired:
     tgt_mask and query_mask are one aliased [num_steps, num_steps] tensor (model.py:117) passed whole as the content mask
     against L < num_steps content tokens (model.py:154-167).  The script asserts that it raises, then mints those modes with
     `forward_ext` below — the same loop around the reference's unmodified `model.decode` / `model.head`, refinement with
     tgt_mask[:L, :L] — and flags them "reference_forward_raises" in the json (a documented extension, not parity);
  5. records one teacher-forced `model.decode` with the content / query mask pair of one permutation drawn by the reference's
     `gen_tgt_perms` / `generate_attn_masks`, and the reference's evaluation-mode permutation loss (`training_step` under
     .eval()) for the permutations drawn.

Usage:  python tools/make_golden_dec_depth.py --ref <reference checkout> [--out tests/golden]
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.make_golden import min_margin  # noqa: E402
from oracle.make_golden_hub import modes_for  # noqa: E402
from oracle.make_golden_train import install_stubs  # noqa: E402
from oracle.synth import CHARSET_36, CONFIGS, charset_config, state_dict_fingerprint, synth_images, synth_state_dict  # noqa: E402

# name -> (experiment, keyword overrides of create_model, EOS bias of the synthetic head, weight seed)
DEC_DEPTH_VARIANTS = {
    'parseq_dec2': ('parseq', {'dec_depth': 2}, 3.0, 0),
    'parseq-tiny_c36_len10_dec3': ('parseq-tiny', {'dec_depth': 3, 'charset_train': CHARSET_36, 'max_label_length': 10}, 0.75, 0),
}
MEMORY_ROWS = 32                                 # tokens of the first crop's `memory` stored in full
LABELS = ['Hello', 'a7', 'MI355X', 'x7b']       # teacher-forced decode / permutation loss (filtered to the variant's charset)


def dec_depth_config(name: str):
    experiment, kw, _, _ = DEC_DEPTH_VARIANTS[name]
    base = dataclasses.replace(CONFIGS[experiment], dec_depth=kw['dec_depth'])
    if 'charset_train' in kw:
        extra = {'max_label_length': kw['max_label_length']} if 'max_label_length' in kw else {}
        return charset_config(base, kw['charset_train'], **extra)
    return base


def dec_depth_state_dict(name: str):
    _, _, eos_bias, seed = DEC_DEPTH_VARIANTS[name]
    return synth_state_dict(dec_depth_config(name), seed, eos_bias=eos_bias)


def modes_with_full(max_label_length: int):
    modes = modes_for(max_label_length)
    modes['ar1_full'] = (True, 1, max_label_length)
    return modes


@torch.inference_mode()
def forward_ext(model, tokenizer, images, max_length=None):
    """model.py:105-169 around the reference's own `encode` / `decode` / `head`, except that refinement passes the content mask
    restricted to the L content positions that exist, tgt_mask[:L, :L] — what the reference computes whenever it does not raise."""
    testing = max_length is None
    max_length = model.max_label_length if max_length is None else min(max_length, model.max_label_length)
    bs = images.shape[0]
    num_steps = max_length + 1
    memory = model.encode(images)
    pos_queries = model.pos_queries[:, :num_steps].expand(bs, -1, -1)
    tgt_mask = query_mask = torch.triu(torch.ones((num_steps, num_steps), dtype=torch.bool), 1)
    if model.decode_ar:
        tgt_in = torch.full((bs, num_steps), tokenizer.pad_id, dtype=torch.long)
        tgt_in[:, 0] = tokenizer.bos_id
        logits = []
        for i in range(num_steps):
            j = i + 1
            tgt_out = model.decode(tgt_in[:, :j], memory, tgt_mask[:j, :j], tgt_query=pos_queries[:, i:j], tgt_query_mask=query_mask[i:j, :j])
            p_i = model.head(tgt_out)
            logits.append(p_i)
            if j < num_steps:
                tgt_in[:, j] = p_i.squeeze().argmax(-1)
                if testing and (tgt_in == tokenizer.eos_id).any(dim=-1).all():
                    break
        logits = torch.cat(logits, dim=1)
    else:
        tgt_in = torch.full((bs, 1), tokenizer.bos_id, dtype=torch.long)
        logits = model.head(model.decode(tgt_in, memory, tgt_query=pos_queries))
    if model.refine_iters:
        query_mask[torch.triu(torch.ones(num_steps, num_steps, dtype=torch.bool), 2)] = 0
        bos = torch.full((bs, 1), tokenizer.bos_id, dtype=torch.long)
        for _ in range(model.refine_iters):
            tgt_in = torch.cat([bos, logits[:, :-1].argmax(-1)], dim=1)
            L = tgt_in.shape[1]
            tgt_padding_mask = (tgt_in == tokenizer.eos_id).int().cumsum(-1) > 0
            tgt_out = model.decode(tgt_in, memory, tgt_mask[:L, :L], tgt_padding_mask, pos_queries, query_mask[:, :L])
            logits = model.head(tgt_out)
    return logits


@torch.inference_mode()
def run_mode(system, images, mode):
    decode_ar, refine_iters, max_length = mode
    system.model.decode_ar, system.model.refine_iters = decode_ar, refine_iters
    return system.forward(images, max_length)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', required=True, help='checkout of the reference repository')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    ap.add_argument('--candidates', type=int, default=64)
    ap.add_argument('--keep', type=int, default=4)
    args = ap.parse_args()
    from safetensors.torch import save_file
    install_stubs()
    sys.path.insert(0, args.ref)
    from strhub.models import utils as ref_utils

    for name, (experiment, kwargs, eos_bias, seed) in DEC_DEPTH_VARIANTS.items():
        cfg = dec_depth_config(name)
        resolved = ref_utils._get_config(experiment, **kwargs)
        torch.manual_seed(0)
        system = ref_utils.create_model(experiment, **kwargs).eval()
        tok = system.tokenizer
        assert len(tok) == cfg.num_tokens and (tok.eos_id, tok.bos_id, tok.pad_id) == (cfg.eos_id, cfg.bos_id, cfg.pad_id)
        assert len(system.model.decoder.layers) == cfg.dec_depth and system.model.max_label_length == cfg.max_label_length
        sd = dec_depth_state_dict(name)
        assert list(sd) == list(system.model.state_dict()), 'synthetic state dict order != the reference model\'s'
        res = system.model.load_state_dict(sd, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        modes = modes_with_full(cfg.max_label_length)
        npos = cfg.max_label_length + 1

        # crops: best-separated among those whose AR string ends strictly inside the label range, distinct end positions first
        cand = synth_images(args.candidates, cfg, seed=4321)
        worst = torch.full((args.candidates,), float('inf'))
        for mode in ('nar0', 'ar0_full', 'nar1', 'ar1_full'):
            worst = torch.minimum(worst, min_margin(run_mode(system, cand, modes[mode])))
        ar_ids = run_mode(system, cand, modes['ar0_full']).argmax(-1)
        is_eos = ar_ids == tok.eos_id
        first = torch.where(is_eos.any(-1), is_eos.int().argmax(-1), torch.full((args.candidates,), npos))
        inside = [i for i in ((first >= 1) & (first < npos - 1)).nonzero().flatten().tolist() if float(worst[i]) > 1e-3]
        inside.sort(key=lambda i: -float(worst[i]))
        chosen, ends = [], set()
        for i in inside:                           # one crop per end position first ...
            if len(chosen) < args.keep and int(first[i]) not in ends:
                chosen.append(i); ends.add(int(first[i]))
        for i in inside:                           # ... then the best-separated of the rest
            if len(chosen) < args.keep and i not in chosen:
                chosen.append(i)
        assert len(chosen) == args.keep and len(ends) >= 2, (name, 'not enough crops with a mixed early exit', first.tolist())
        order = torch.tensor(sorted(chosen))
        images = cand[order].contiguous()
        out = {'images': images}
        with torch.inference_mode():
            memory = system.model.encode(images).contiguous()
        # `memory` in full would make the file large: the first crop's first MEMORY_ROWS tokens in full, every crop's norm in the json
        out['memory.head'] = memory[0, :MEMORY_ROWS].contiguous()
        meta = {'model': name, 'experiment': experiment, 'kwargs': kwargs, 'eos_bias': eos_bias, 'seed': seed,
                'resolved_config': resolved, 'state_dict_keys': list(sd), 'num_params': sum(p.numel() for p in system.model.parameters()),
                'candidate_ids': order.tolist(), 'sd_fingerprint': state_dict_fingerprint(sd), 'min_margin': float(worst[order].min()),
                'tokenizer': {'len': len(tok), 'eos_id': tok.eos_id, 'bos_id': tok.bos_id, 'pad_id': tok.pad_id},
                'memory_norms': [float(n) for n in memory.double().flatten(1).norm(dim=1)], 'torch': torch.__version__, 'modes': {}}
        for mode, spec in modes.items():
            raises = False
            try:
                logits = run_mode(system, images, spec)
            except RuntimeError:
                raises = True
            decode_ar, refine_iters, max_length = spec
            if decode_ar and refine_iters and max_length is None:
                assert raises, (name, mode, 'the reference forward was expected to raise after the early exit')
            else:
                assert not raises, (name, mode)
            if raises:
                system.model.decode_ar, system.model.refine_iters = decode_ar, refine_iters
                logits = forward_ext(system.model, tok, images, max_length)
            else:     # the restatement reproduces the reference wherever the reference is defined
                system.model.decode_ar, system.model.refine_iters = decode_ar, refine_iters
                assert torch.equal(forward_ext(system.model, tok, images, max_length), logits), (name, mode)
            out[f'logits.{mode}'] = logits.contiguous()
            strings, probs = tok.decode(logits.softmax(-1))
            meta['modes'][mode] = {'decode_ar': decode_ar, 'refine_iters': refine_iters, 'max_length': max_length, 'shape': list(logits.shape),
                                   'strings': strings, 'confidence': [float(p.prod()) for p in probs], 'reference_forward_raises': raises}
            if raises:
                meta['modes'][mode]['definition'] = 'refinement with the content mask tgt_mask[:L, :L] (documented extension, not parity)'

        # teacher-forced decode with one permutation's (content, query) mask pair, and the evaluation-mode permutation loss
        labels = [''.join(ch for ch in lab if ch in tok._stoi)[:cfg.max_label_length] or 'a' for lab in LABELS]
        system.rng = np.random.default_rng(11)
        torch.manual_seed(22)
        drawn = []
        gen = system.gen_tgt_perms
        system.gen_tgt_perms = lambda tgt: drawn.append(gen(tgt)) or drawn[-1]
        with torch.no_grad():
            loss = system.training_step((images, labels), 0)
        system.gen_tgt_perms = gen
        perms = drawn[0]
        tgt = tok.encode(labels)
        tgt_in = tgt[:, :-1]
        padding = (tgt_in == tok.pad_id) | (tgt_in == tok.eos_id)
        k = min(2, perms.shape[0] - 1)
        cmask, qmask = system.generate_attn_masks(perms[k])
        with torch.inference_mode():
            hidden = system.model.decode(tgt_in, memory, cmask, padding, tgt_query_mask=qmask)
            out['tf.logits'] = system.model.head(hidden).contiguous()
        out['tf.hidden'] = hidden.contiguous()
        out['tf.tgt_in'] = tgt_in.to(torch.int32).contiguous()
        out['tf.padding'] = padding.to(torch.uint8).contiguous()
        out['tf.content_mask'] = cmask.to(torch.uint8).contiguous()
        out['tf.query_mask'] = qmask.to(torch.uint8).contiguous()
        out['perms'] = perms.to(torch.int32).contiguous()
        out['loss'] = loss.detach().reshape(1).float()
        meta['teacher_forced'] = {'labels': labels, 'perm_index': k, 'loss': float(loss), 'num_perms': int(perms.shape[0])}
        save_file(out, os.path.join(args.out, f'{name}.safetensors'))
        with open(os.path.join(args.out, f'{name}.json'), 'w') as f:
            json.dump(meta, f, indent=1)
        print(name, 'params', meta['num_params'], 'kept', order.tolist(), 'ends', sorted(int(first[i]) for i in chosen),
              'min margin', meta['min_margin'], 'loss', float(loss))
        for mode in modes:
            print('  ', mode, meta['modes'][mode]['shape'], meta['modes'][mode]['strings'], meta['modes'][mode]['reference_forward_raises'])


if __name__ == '__main__':
    main()
