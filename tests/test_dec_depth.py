"""PARSeq decoders deeper than one layer (`dec_depth` > 1), which the reference accepts through its hub keyword arguments
(`create_model('parseq', dec_depth=2)`; `Decoder` clones the layer, modules.py:101-125).  Layers 0 .. D-2 update the content stream
under the content mask and layers 1 .. D-1 attend to that updated content (modules.py:116-124).

Goldens: tools/make_golden_dec_depth.py runs the reference's UNMODIFIED create_model / forward / decode / training_step
(tests/golden/parseq_dec2.*, parseq-tiny_c36_len10_dec3.*).  Where the reference's forward raises (AR in testing mode with refinement
after the batch-level early exit), the vectors follow the definition of DESIGN.md section 9 — refinement with tgt_mask[:L, :L] — and
are flagged `reference_forward_raises`.

CPU: resolved configuration, the hub entry, the state_dict key order, the training entry points refusing a deeper decoder.
GPU: every decode mode against the goldens; teacher-forced decode with a content mask and the permutation loss; a depth-2 decoder
whose second layer adds nothing equals the depth-1 decoder; the cached AR loop equals a full recompute; the small-batch route."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from make_golden_dec_depth import DEC_DEPTH_VARIANTS, dec_depth_config, dec_depth_state_dict, modes_with_full  # noqa: E402
from oracle.synth import state_dict_fingerprint, synth_images  # noqa: E402

VARIANTS = list(DEC_DEPTH_VARIANTS)
MODE_NAMES = ['nar0', 'nar1', 'ar0', 'ar0_full', 'ar0_short', 'ar1', 'ar2', 'ar1_full']
DEV = 'cuda'


def _build(variant, precision=None, sd=None, **overrides):
    from parseq_amd import create_model
    experiment, kwargs, _, _ = DEC_DEPTH_VARIANTS[variant]
    kw = dict(kwargs, **overrides)
    if precision is not None:
        kw['precision'] = precision
    m = create_model(experiment, **kw)
    m.model.load_state_dict(dec_depth_state_dict(variant) if sd is None else sd, strict=True)
    return m.eval()


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('variant', VARIANTS)
def test_resolved_config_equals_the_references(variant, golden):
    from parseq_amd.configs import get_config
    _, meta = golden(variant)
    experiment, kwargs, eos_bias, seed = DEC_DEPTH_VARIANTS[variant]
    assert (meta['experiment'], meta['eos_bias'], meta['seed']) == (experiment, eos_bias, seed)
    ours, ref = get_config(experiment, **kwargs), meta['resolved_config']
    assert set(ours) == set(ref), set(ours) ^ set(ref)
    for k in ref:
        assert ours[k] == ref[k], (k, ours[k], ref[k])


@pytest.mark.parametrize('variant', VARIANTS)
def test_hub_entry_state_dict_and_weights(variant, golden):
    """The hub entry builds the depth the keyword asks for, with the reference's state_dict keys in the reference's order; the
    synthetic weights regenerate bit for bit (fingerprint)."""
    import hubconf
    _, meta = golden(variant)
    experiment, kwargs, _, _ = DEC_DEPTH_VARIANTS[variant]
    entry = {'parseq': hubconf.parseq, 'parseq-tiny': hubconf.parseq_tiny}[experiment]
    m = entry(pretrained=False, **kwargs)
    assert m.hparams['dec_depth'] == kwargs['dec_depth'] == len(m.model.decoder.layers)
    assert list(m.model.state_dict()) == meta['state_dict_keys']
    assert sum(p.numel() for p in m.model.parameters()) == meta['num_params']
    sd = dec_depth_state_dict(variant)
    assert state_dict_fingerprint(sd) == meta['sd_fingerprint']
    res = m.model.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    tok = m.tokenizer
    assert {'len': len(tok), 'eos_id': tok.eos_id, 'bos_id': tok.bos_id, 'pad_id': tok.pad_id} == meta['tokenizer']


def test_goldens_flag_the_modes_where_the_reference_raises(golden):
    """AR in testing mode with refinement raises in the reference after an early exit; every other mode is the reference's own forward."""
    for variant in VARIANTS:
        _, meta = golden(variant)
        for mode, spec in meta['modes'].items():
            assert spec['reference_forward_raises'] == (mode in ('ar1', 'ar2')), (variant, mode)
        assert meta['modes']['ar0']['shape'][1] < meta['modes']['ar0_full']['shape'][1]      # the early exit fired


def test_training_entry_points_refuse_a_deeper_decoder():
    from parseq_amd import train
    m = _build('parseq_dec2')
    images = torch.zeros(2, 3, 32, 128)
    labels = ['ab', 'c']
    calls = {
        'training_step_loss': lambda: train.training_step_loss(m, images, labels),
        'TrainStep': lambda: train.TrainStep(m, total_steps=10),
        'loss_and_grads': lambda: train.loss_and_grads(m, images, labels),
        'loss_and_grads_micro': lambda: train.loss_and_grads_micro(m, images, labels),
        'decoder_backward': lambda: train.decoder_backward(m, images, labels),
        'system.training_step': lambda: m.training_step((images, labels), 0),
    }
    for name, call in calls.items():
        with torch.enable_grad(), pytest.raises(ValueError, match='dec_depth'):
            call()


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------

def _run(m, images, spec, **kw):
    m.model.decode_ar, m.model.refine_iters = spec['decode_ar'], spec['refine_iters']
    with torch.inference_mode():
        out = m(images, spec['max_length'], **kw)
    torch.cuda.synchronize()
    return out.float().cpu()


def _check(tag, m, got, ref, spec, tol=1e-3, rows=None):
    from gpu_util import report
    assert list(got.shape[1:]) == spec['shape'][1:] and got.shape == ref.shape, (tag, got.shape, ref.shape)
    err, msg = report(tag, got, ref)
    assert err <= tol, msg
    assert torch.equal(got.argmax(-1), ref.argmax(-1)), msg
    strings, probs = m.tokenizer.decode(got.softmax(-1))
    want = spec['strings'] if rows is None else spec['strings'][:rows]
    assert strings == want, msg
    conf = torch.tensor([float(p.prod()) for p in probs])
    want_conf = torch.tensor(spec['confidence'] if rows is None else spec['confidence'][:rows])
    assert torch.allclose(conf, want_conf, rtol=2e-3, atol=1e-6), msg


def _check_bf16(tag, got, ref):
    """bf16 operands: 6e-2 of the exact reference (tests/test_hip_parity.py's bar), decisions identical up to the first near-tie."""
    from gpu_util import report
    assert got.shape == ref.shape
    err, msg = report(tag, got, ref)
    top2 = ref.topk(2, -1).values
    safe = ((top2[..., 0] - top2[..., 1]) > 0.12).int().cumprod(-1).bool()
    assert torch.isfinite(got).all() and bool((got.argmax(-1) == ref.argmax(-1))[safe].all()), msg
    assert (got - ref).abs()[safe].max().item() <= 6e-2 if bool(safe.any()) else True, msg


@pytest.fixture(scope='module')
def models():
    cache = {}

    def get(variant, precision):
        if (variant, precision) not in cache:
            cache[(variant, precision)] = _build(variant, precision).to(DEV)
        return cache[(variant, precision)]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize('precision', ['fp32', 'bf16x3', 'bf16'])
@pytest.mark.parametrize('variant', VARIANTS)
def test_forward_matches_reference(variant, precision, models, golden):
    """Every decode mode (AR, NAR, refinement, early exit, max_length; 'ar1_full' is AR + 1 refinement where the reference's own forward
    runs, pinning the early-exit definition of ar1 / ar2 where the reference is defined)."""
    g, meta = golden(variant)
    m = models(variant, precision)
    images = g['images'].to(DEV)
    outs = {}
    for mode in MODE_NAMES:
        spec = meta['modes'][mode]
        got, ref = _run(m, images, spec), g[f'logits.{mode}']
        outs[mode] = got
        if precision != 'bf16':
            _check(f'{variant} {precision} {mode}', m, got, ref, spec)
        elif mode not in _PREVIOUS_PASS:
            _check_bf16(f'{variant} bf16 {mode}', got, ref)
        else:
            # a refinement reads the previous pass's decisions as its context: compare the crops whose context equals the reference's
            prev = _PREVIOUS_PASS[mode]
            same = [b for b in range(got.shape[0]) if _context(outs[prev][b], meta['tokenizer']['eos_id']) ==
                    _context(g[f'logits.{prev}'][b], meta['tokenizer']['eos_id'])]
            assert torch.isfinite(got).all() and got.shape == ref.shape
            if same:
                _check_bf16(f'{variant} bf16 {mode} crops {same}', got[same], ref[same])


# the pass whose arg-max a refinement mode takes as its content tokens (model.py:161)
_PREVIOUS_PASS = {'nar1': 'nar0', 'ar1': 'ar0_full', 'ar1_full': 'ar0_full', 'ar2': 'ar1'}


def _context(logits, eos_id):
    """The refinement context a pass leaves: its decisions up to and including the first EOS (the rest is key-padded)."""
    ids = logits[:-1].argmax(-1).tolist()
    return ids[:ids.index(eos_id) + 1] if eos_id in ids else ids


@pytest.mark.gpu
@pytest.mark.parametrize('variant', VARIANTS)
def test_encoder_memory(variant, models, golden):
    """The encoder output the deeper decoder's K / V are projected from: the stored slice (first crop, first tokens) and every crop's norm."""
    from gpu_util import report
    g, meta = golden(variant)
    for precision, tol in (('fp32', 2e-4), ('bf16x3', 5e-4)):
        with torch.inference_mode():
            mem = models(variant, precision).model.encode(g['images'].to(DEV)).double().cpu()
        head = g['memory.head']
        err, msg = report(f'{variant} memory {precision}', mem[0, :head.shape[0]].float(), head)
        assert err <= tol, msg
        norms = mem.flatten(1).norm(dim=1)
        assert torch.allclose(norms, torch.tensor(meta['memory_norms'], dtype=torch.float64), rtol=1e-5), (norms, meta['memory_norms'])


@pytest.mark.gpu
@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('variant', VARIANTS)
def test_teacher_forced_decode_and_permutation_loss(variant, precision, models, golden):
    """model.decode with the content / query masks of one permutation (the content mask is what a deeper decoder reads), and the
    evaluation-mode permutation loss of the reference's training_step for the permutations it drew."""
    from gpu_util import report
    from parseq_amd.system import permutation_loss
    g, meta = golden(variant)
    m = models(variant, precision)
    images = g['images'].to(DEV)
    with torch.inference_mode():
        memory = m.model.encode(images)
        hidden = m.model.decode(g['tf.tgt_in'].long().to(DEV), memory, g['tf.content_mask'].bool().to(DEV), g['tf.padding'].bool().to(DEV),
                                tgt_query_mask=g['tf.query_mask'].bool().to(DEV))
        logits = m.model.head(hidden)
    for tag, got, ref in (('hidden', hidden, g['tf.hidden']), ('logits', logits, g['tf.logits'])):
        err, msg = report(f'{variant} {precision} teacher-forced {tag}', got.float().cpu(), ref)
        assert err <= 1e-3, msg
    # without the content mask the content stream sees every position: the result must change (the mask is really read)
    with torch.inference_mode():
        unmasked = m.model.decode(g['tf.tgt_in'].long().to(DEV), memory, None, g['tf.padding'].bool().to(DEV),
                                  tgt_query_mask=g['tf.query_mask'].bool().to(DEV))
    assert (unmasked.float().cpu() - g['tf.hidden']).abs().max().item() > 1e-3
    with torch.no_grad():
        loss = permutation_loss(m, images, meta['teacher_forced']['labels'], g['perms'].long())[0]
    assert abs(float(loss) - float(g['loss'])) <= 1e-3, (float(loss), float(g['loss']))


@pytest.mark.gpu
@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
def test_inert_second_layer_equals_depth_one(precision, monkeypatch):
    """A depth-2 decoder whose layer 1 adds nothing to the residual stream (out_proj of both attentions and linear2 zero) is the
    depth-1 decoder of the same layer 0, in every mode, at batch 512 with distinct crops.  The depth-1 side runs the per-op AR step and
    the encoder without its fused tail — the kernels the deeper decoder composes."""
    monkeypatch.setenv('PARSEQ_NO_FUSED_STEP', '1')
    monkeypatch.setenv('PARSEQ_NO_FUSED_TAIL', '1')
    sd2 = dec_depth_state_dict('parseq_dec2')
    for k in list(sd2):
        if k.startswith('decoder.layers.1.') and any(s in k for s in ('out_proj.', 'linear2.')):
            sd2[k] = torch.zeros_like(sd2[k])
    sd1 = {k: v for k, v in sd2.items() if not k.startswith('decoder.layers.1.')}
    deep = _build('parseq_dec2', precision, sd=sd2).to(DEV)
    one = _build('parseq_dec2', precision, sd=sd1, dec_depth=1).to(DEV)
    images = synth_images(512, dec_depth_config('parseq_dec2'), seed=777).to(DEV)
    for mode, (decode_ar, refine_iters, max_length) in modes_with_full(25).items():
        spec = {'decode_ar': decode_ar, 'refine_iters': refine_iters, 'max_length': max_length}
        a, b = _run(deep, images, spec), _run(one, images, spec)
        assert a.shape == b.shape, (mode, a.shape, b.shape)
        d = (a - b).abs().max().item()
        assert d <= 1e-5, (precision, mode, d)
        assert deep.tokenizer.decode(a.softmax(-1))[0] == one.tokenizer.decode(b.softmax(-1))[0], (precision, mode)


@pytest.mark.gpu
@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('variant', VARIANTS)
def test_cached_ar_loop_equals_full_recompute(variant, precision, models):
    """The AR loop computes one content row per layer and step and appends it to the per-layer cache; a teacher-forced decode of its
    own output tokens under the causal content / query masks recomputes every position of every layer (what the reference does at each
    step): the logits must agree, at batch 512."""
    from gpu_util import report
    m = models(variant, precision)
    cfg = dec_depth_config(variant)
    npos = cfg.max_label_length + 1
    images = synth_images(512, cfg, seed=99).to(DEV)
    ar = _run(m, images, {'decode_ar': True, 'refine_iters': 0, 'max_length': cfg.max_label_length})
    tgt_in = torch.cat([torch.full((512, 1), cfg.bos_id, dtype=torch.long), ar[:, :-1].argmax(-1)], dim=1).to(DEV)
    causal = torch.triu(torch.ones(npos, npos, dtype=torch.bool, device=DEV), 1)
    with torch.inference_mode():
        full = m.model.head(m.model.decode(tgt_in, None, causal, None, tgt_query_mask=causal)).float().cpu()
    err, msg = report(f'{variant} {precision} AR cache vs full recompute', ar, full)
    assert err <= 1e-3, msg


@pytest.mark.gpu
@pytest.mark.small_batch_route
@pytest.mark.parametrize('variant', VARIANTS)
def test_small_batch_route(variant, golden):
    """Batches of 1 and 3 crops through the library's default small-batch route (per-operation encoder), bf16x3: the modes whose rows do
    not depend on the rest of the batch against the goldens' rows."""
    g, meta = golden(variant)
    m = _build(variant, 'bf16x3').to(DEV)
    for n in (1, 3):
        images = g['images'][:n].contiguous().to(DEV)
        for mode in ('nar0', 'nar1', 'ar0_full', 'ar0_short', 'ar1', 'ar2', 'ar1_full'):
            spec = meta['modes'][mode]
            _check(f'{variant} batch {n} {mode}', m, _run(m, images, spec), g[f'logits.{mode}'][:n], spec, rows=n)


@pytest.mark.gpu
def test_depth_outside_the_supported_range_is_rejected():
    from parseq_amd._native import NativeError
    from parseq_amd import create_model
    m = create_model('parseq-tiny', dec_depth=5).eval().to(DEV)
    with pytest.raises(NativeError, match='dec_depth=5'), torch.inference_mode():
        m(torch.zeros(1, 3, 32, 128, device=DEV))
