"""GPU tests of N-best evaluation: `parseq_eval_beams` against the CPU restatement (tests/beam_eval_reference.py)
and the reference's `_eval_step` totals, `BeamEvaluator` through every search it wraps, the refusals, test.py and tools/tune_fusion.py."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import beam_eval_reference as R
from gpu_util import DEV, make_model, native
from oracle.synth import CONFIGS, synth_images
from parseq_amd.configs import CHARSET_94_FULL
from parseq_amd.tokenizer import CharsetAdapter, Tokenizer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG_INF = float('-inf')
ACC_WORDS = 28


def new_accum():
    return torch.zeros(ACC_WORDS, dtype=torch.int64, device=DEV)


def read_accum(acc):
    h = acc.cpu()
    ints, floats = h[:25].tolist(), h[25:].view(torch.float64).tolist()
    out = dict(zip(R.INT_NAMES, ints[:8]))
    out['first_hit'] = ints[8:]
    out.update(zip(R.FLOAT_NAMES, floats))
    return out


def run_operator(case, table, classes, G, acc, stream=None):
    """One call of the entry point on a synthetic N-best (nested lists).  Returns the outputs on the host; `acc` is accumulated into."""
    nat, lib = native()
    tokens, scores, lengths, confs, labels = case
    B, W, T = len(tokens), len(tokens[0]), len(tokens[0][0])
    d_tokens = torch.tensor(tokens, dtype=torch.int32, device=DEV)
    d_scores = torch.tensor(scores, dtype=torch.float32, device=DEV)
    d_lengths = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    d_confs = torch.tensor(confs, dtype=torch.float32, device=DEV)
    gt = np.full((B, G), 0x7e, dtype=np.int32)                     # the padding is a character of every charset here: it must not be read
    for b, label in enumerate(labels):
        gt[b, :len(label)] = [ord(c) for c in label]
    d_gt = torch.from_numpy(gt).to(DEV)
    d_len = torch.tensor([len(y) for y in labels], dtype=torch.int32, device=DEV)
    tab = torch.as_tensor(table, dtype=torch.int32).to(DEV)
    hyp = torch.full((B * W, 4), -7, dtype=torch.int32, device=DEV)
    img = torch.full((B, 8), -7, dtype=torch.int32, device=DEV)
    ws = torch.full((B * (W + 3),), -7.0, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream) if stream is not None else nat.guard(d_tokens):
        nat.check(lib.parseq_eval_beams(nat.ptr(d_tokens), nat.ptr(d_scores), nat.ptr(d_lengths), nat.ptr(d_confs), B, W, T, classes, nat.ptr(tab),
                                        nat.ptr(d_gt), nat.ptr(d_len), G, nat.ptr(hyp), nat.ptr(img), nat.ptr(ws), nat.ptr(acc), nat.stream_ptr(d_tokens)))
    torch.cuda.synchronize()
    ws = ws.cpu()
    return dict(hyp_rows=hyp.cpu().tolist(), image_rows=img.cpu().tolist(), hyp_ned=ws[:B * W].tolist(), image_ned=ws[B * W:B * W + B].tolist(),
                image_oracle_ned=ws[B * W + B:B * W + 2 * B].tolist(), image_confidence=ws[B * W + 2 * B:].tolist())


def rounded(case):
    """The case with its scores as the fp32 values the device sees."""
    tokens, scores, lengths, confs, labels = case
    f32 = lambda rows: np.asarray(rows, dtype=np.float32).astype(np.float64).tolist()
    return tokens, f32(scores), lengths, f32(confs), labels


def charsets(C):
    """(tokenizer, adapter, test charset) of the synthetic cases: C = 37 drops x, y, z; C = 95 folds the case and drops the punctuation."""
    if C == 37:
        test = ''.join(c for c in R.CHARSET_36 if c not in R.DROPPED_36)
        return Tokenizer(R.CHARSET_36), CharsetAdapter(test), test
    return Tokenizer(CHARSET_94_FULL), CharsetAdapter(R.CHARSET_36), R.CHARSET_36


def table_of(tok, adapter):
    from parseq_amd.evaluate import adapter_table
    table = adapter_table(tok, adapter)
    assert table is not None
    return table


def close(got, want, rel):
    return abs(got - want) <= rel * abs(want)


# The rows kernel runs four waves (four hypotheses) per workgroup: B * W = 1, 5, 514 and 4369 leave idle waves in the last one.  The image kernel is
# one workgroup of 256 threads: B = 257 puts image 256 on thread 0's second stride.  G = 64 / 65 / 256 end on, one past and four times the 64
# wide text blocks of the recurrence; T = 32 is the widest pattern; W = 17 the widest list.
OPERATOR_CASES = [(1, 1, 1, 1, 37), (1, 1, 26, 25, 95), (4, 1, 32, 256, 95), (5, 1, 26, 64, 37), (257, 2, 26, 25, 37), (257, 16, 26, 65, 95),
                  (257, 17, 32, 256, 37)]


@pytest.mark.parametrize('B,W,T,G,C', OPERATOR_CASES)
def test_operator_equals_the_restatement(B, W, T, G, C):
    tok, adapter, test = charsets(C)
    case = rounded(R.synthetic_case(B, W, T, G, tok, test, np.random.default_rng(B * 1000 + W * 10 + T)))
    want = R.evaluate(*case, tok, adapter)
    if W >= 2:
        assert R.coverage_holds(want, W), (want['totals'], want['first_hit'])
        assert R.kinds_present(case, want, tok, adapter)
    acc = new_accum()
    got = run_operator(case, table_of(tok, adapter), C, G, acc)
    for key in ('hyp_rows', 'image_rows', 'hyp_ned', 'image_ned', 'image_oracle_ned'):
        assert got[key] == want[key], key
    for g, w in zip(got['image_confidence'], want['image_confidence']):
        assert close(g, w, 1e-15 * 4)                                # one double exp on each side, each within an ulp
    totals = read_accum(acc)
    print((B, W, T, G, C), totals)
    assert [totals[k] for k in R.INT_NAMES] == [want['totals'][k] for k in R.INT_NAMES] and totals['first_hit'] == want['first_hit']
    for k in R.FLOAT_NAMES:
        assert close(totals[k], want['totals'][k], 1e-12), k


def test_totals_accumulate_and_repeat_bit_for_bit():
    tok, adapter, test = charsets(95)
    table = table_of(tok, adapter)
    rng = np.random.default_rng(17)
    cases = [rounded(R.synthetic_case(B, 5, 26, 25, tok, test, rng)) for B in (257, 5, 130)]
    want = R.add_totals([R.evaluate(*case, tok, adapter) for case in cases])
    accs = []
    side = torch.cuda.Stream()
    for stream in (None, None, side):
        acc = new_accum()
        for case in cases:
            run_operator(case, table, 95, 25, acc, stream)
        accs.append(acc.cpu())
    got = read_accum(accs[0])
    print(got, want)
    assert [got[k] for k in R.INT_NAMES] == [want[k] for k in R.INT_NAMES] and got['first_hit'] == want['first_hit']
    for k in R.FLOAT_NAMES:
        assert close(got[k], want[k], 1e-12), k
    assert torch.equal(accs[0], accs[1]) and torch.equal(accs[0], accs[2])


@pytest.mark.parametrize('name', ['c94_c36', 'c94_c94', 'c36_c36', 'c200_c174'])
def test_width_one_equals_the_reference_eval_step(name, golden):
    """W = 1 results made on the host from the fixture's stored logits: arg-max ids cut at <eos>, score = log of the reference's confidence."""
    tensors, meta = golden('eval_metrics')
    case = meta['cases'][name]
    tok = Tokenizer(case['charset_train'])
    table = table_of(tok, CharsetAdapter(case['charset_test']))
    logits = tensors[f'{name}.q'].to(torch.float32) * 0.25
    tokens, lengths = [], []
    for row_ids in logits.argmax(-1).tolist():
        tokens.append([row_ids]); lengths.append([row_ids.index(tok.eos_id) if tok.eos_id in row_ids else len(row_ids)])
    acc = new_accum()
    scores = np.log(np.asarray(case['row_confidence'], dtype=np.float32)).reshape(-1, 1).tolist()      # an fp32 log
    run_operator((tokens, scores, lengths, scores, case['labels']), table, len(tok) - 2, max(map(len, case['labels'])), acc)
    got, want = read_accum(acc), case['result']
    print(name, got, want)
    assert (got['num_samples'], got['correct'], got['label_length']) == (want['num_samples'], want['correct'], want['label_length'])
    assert close(got['ned'], want['ned'], 1e-9)
    assert close(got['confidence'], want['confidence'], 1e-6)


def test_operator_refusals_leave_everything_untouched():
    nat, lib = native()
    B, W, T, G, C = 3, 2, 8, 6, 37
    t = dict(tokens=torch.zeros(B, W, 32, dtype=torch.int32, device=DEV), scores=torch.zeros(B, W, device=DEV),
             lengths=torch.zeros(B, W, dtype=torch.int32, device=DEV), confs=torch.zeros(B, W, device=DEV),
             table=torch.zeros(C, dtype=torch.int32, device=DEV), gt=torch.zeros(B, 300, dtype=torch.int32, device=DEV),
             gt_len=torch.ones(B, dtype=torch.int32, device=DEV))
    hyp = torch.full((B * 20, 4), -7, dtype=torch.int32, device=DEV)
    img = torch.full((B, 8), -7, dtype=torch.int32, device=DEV)
    ws = torch.full((B * 23,), -7.0, dtype=torch.float64, device=DEV)
    acc = torch.full((ACC_WORDS,), 0x5a5a5a5a, dtype=torch.int64, device=DEV)
    keep = [x.clone() for x in (hyp, img, ws, acc)]
    names = ['tokens', 'scores', 'lengths', 'confs', 'table', 'gt', 'gt_len']

    def call(shape=(B, W, T, G), null=None):
        b, w, steps, g = shape
        p = {k: (None if k == null else nat.ptr(v)) for k, v in t.items()}
        outs = [None if null == k else nat.ptr(v) for k, v in (('hyp', hyp), ('img', img), ('ws', ws), ('acc', acc))]
        return lib.parseq_eval_beams(p['tokens'], p['scores'], p['lengths'], p['confs'], b, w, steps, C, p['table'], p['gt'], p['gt_len'], g, *outs,
                                     nat.stream_ptr(hyp))

    bad = [((B, 0, T, G), b'W'), ((B, 18, T, G), b'W'), ((B, W, 0, G), b'T'), ((B, W, 33, G), b'T'), ((B, W, T, 0), b'G'), ((B, W, T, 257), b'G'),
           ((0, W, T, G), b'B'), ((-1, W, T, G), b'B')]
    for shape, word in bad:
        assert call(shape) == -1 and word in lib.parseq_last_error(), shape
    for null in names + ['hyp', 'img', 'ws', 'acc']:
        assert call(null=null) == -1 and b'null' in lib.parseq_last_error(), null
    torch.cuda.synchronize()
    for now, before in zip((hyp, img, ws, acc), keep):
        assert torch.equal(now, before)
    assert call() == 0                                               # the same buffers are accepted with a good shape
    torch.cuda.synchronize()
    assert not torch.equal(acc, keep[3])


# -------------------------------------------------------------------------------------------------------------------
# BeamEvaluator
# -------------------------------------------------------------------------------------------------------------------
WIDTH = 5


def result_totals(r):
    return [r.num_samples, r.correct, r.label_length_sum, r.top1_distance, r.oracle_correct, r.oracle_distance, r.live, r.miss], list(r.first_hit)


def labels_at_ranks(beams, adapter, width):
    """Labels built from an N-best (`decode_beams`' strings): image i takes the adapted string of its live hypothesis at rank i mod (width + 1);
    rank `width` means a string no hypothesis of the image equals.  Where the string at that rank is empty or equals an earlier one after
    the adapter (a folded duplicate would move the hit to the earlier rank), or the image has no live hypothesis there, the nearest rank
    whose string is new in the list and not empty stands in, so that the hits spread over the ranks as the construction means them to."""
    labels = []
    for i, alts in enumerate(beams):
        strings = [adapter(s) for s, _ in alts]
        usable = [r for r, s in enumerate(strings) if s and s not in strings[:r]]
        rank = i % (width + 1)
        if rank < width and usable:
            labels.append(strings[min(usable, key=lambda r: (abs(r - rank), r))])
        else:
            labels.append(next(c * k for k in range(1, 9) for c in 'qzj7' if c * k not in strings))
    return labels


def own_nbest_labels(model, images, width, **search):
    with torch.inference_mode():
        beams = model.tokenizer.decode_beams(model.beam_search(images, width, **search))
    return labels_at_ranks(beams, model.charset_adapter, width)


def check_evaluator(ev, model, images, labels, result, width):
    """`ev` (already updated with `images` / `result`) against the restatement over decode_beams' strings of `result`."""
    beams = model.tokenizer.decode_beams(result)
    if result.model_scores is not None:
        conf = result.model_scores.cpu().tolist()
        beams = [[(s, c) for (s, _), c in zip(alts, row)] for alts, row in zip(beams, conf)]      # dead beams come last in both
    want = R.evaluate_strings(beams, labels, model.charset_adapter, width)
    got = ev.result()
    ints, first_hit = result_totals(got)
    print(ints, first_hit, want['totals'])
    assert ints == [want['totals'][k] for k in R.INT_NAMES] and first_hit == want['first_hit']
    for g, k in ((got.ned_sum, 'ned'), (got.oracle_ned_sum, 'oracle_ned'), (got.confidence_sum, 'confidence')):
        assert close(g, want['totals'][k], 1e-12) or want['totals'][k] == 0 == g
    assert ev.per_sample().tolist() == want['image_rows'] and ev.per_hypothesis().reshape(-1, 4).tolist() == want['hyp_rows']
    return want


def long_reader(name):
    """The synthetic weights with the head's <eos> bias at 0 instead of 2.5: with 2.5 PARSeq-S ends most hypotheses at once, the adapted
    top-1 of every crop is the empty string and no label can stand at rank 0."""
    from oracle.synth import synth_state_dict
    from parseq_amd import create_model
    m = create_model(name, decode_ar=True, refine_iters=1, precision='fp32')
    m.model.load_state_dict(synth_state_dict(CONFIGS[name], 0, eos_bias=0.0))
    return m.eval().to(DEV)


@pytest.fixture(scope='module')
def own_nbest():
    """Per model (fp32, synthetic weights): the crops, the labels built from the plain search's N-best, and the strings of that N-best."""
    out = {}

    def get(name):
        if name not in out:
            model = long_reader(name)
            images = synth_images(3 * (WIDTH + 1), CONFIGS[name], seed=31).to(DEV)
            out[name] = (model, images, own_nbest_labels(model, images, WIDTH))
        return out[name]
    return get


@pytest.mark.parametrize('name', ['parseq-tiny', 'parseq'])
def test_evaluator_on_the_models_own_nbest(name, own_nbest):
    from parseq_amd.evaluate import BeamEvaluator
    model, images, labels = own_nbest(name)
    ev = BeamEvaluator(model, beam_width=WIDTH)
    assert not ev.host_path
    ev.update(images, labels)
    with torch.inference_mode():
        result = model.beam_search(images, WIDTH)
    want = check_evaluator(ev, model, images, labels, result, WIDTH)
    assert R.coverage_holds(want, WIDTH), (want['totals'], want['first_hit'])
    r = ev.result()
    assert r.hit_at(WIDTH) == r.oracle_accuracy == 1 - r.miss / r.num_samples and r.hit_at(1) == r.accuracy
    ev.reset()
    assert ev.result().num_samples == 0


def _lexicon_words(model, images, labels):
    with torch.inference_mode():
        strings = [s for alts in model.tokenizer.decode_beams(model.beam_search(images, WIDTH)) for s, _ in alts]
    words = sorted({w for w in strings + labels if w and all(c in model.tokenizer._stoi for c in w)})
    return words + ['zebra', 'quartz', '0451', 'open', 'exit']


@pytest.mark.parametrize('mode', ['lexicon', 'automaton', 'refine', 'match', 'outside'])
def test_evaluator_through_every_search(mode, own_nbest):
    from parseq_amd.automaton import Automaton
    from parseq_amd.evaluate import BeamEvaluator
    from parseq_amd.lexicon import Lexicon
    model, images, plain_labels = own_nbest('parseq-tiny')
    tok, width = model.tokenizer, WIDTH
    search, match = {}, None
    if mode in ('lexicon', 'automaton', 'match'):
        words = _lexicon_words(model, images, plain_labels)
        if mode == 'automaton':
            counts = [1.0 + (i % 7) for i in range(len(words))]
            search = dict(automaton=Automaton.from_lexicon(words, counts, tok, fold_case=True).to(DEV), alpha=0.5)
        else:
            lexicon = Lexicon(words, tok, fold_case=True, max_label_length=model.model.max_label_length).to(DEV)
            search = dict(lexicon=lexicon)
            match = dict(match=4, keep_reading=True) if mode == 'match' else None
    if mode == 'refine':
        search = dict(refine='score')
    with torch.inference_mode():
        if match:
            result = model.lexicon_match(images, search['lexicon'], 4, keep_reading=True)
        else:
            result = model.beam_search(images, width, **search)
        beams = tok.decode_beams(result)
    slots = result.tokens.shape[1]
    labels = labels_at_ranks(beams, model.charset_adapter, slots)      # from THIS search's N-best, the same construction
    if mode == 'outside':
        ev = BeamEvaluator(model)
        ev.update_result(result, labels)
    else:
        ev = BeamEvaluator(model, beam_width=width, **search, **(match or {}))
        ev.update(images, labels)
    want = check_evaluator(ev, model, images, labels, result, slots)
    assert slots == WIDTH and R.coverage_holds(want, slots), (want['totals'], want['first_hit'])
    assert want['totals']['num_samples'] == len(labels)


@pytest.mark.parametrize('name', ['parseq-tiny', 'parseq'])
def test_width_one_equals_the_greedy_evaluator(name, golden):
    from parseq_amd.evaluate import BeamEvaluator, Evaluator
    g, _ = golden(name)
    m = make_model(name, 'fp32', decode_ar=True, refine_iters=0)
    x = g['images'].to(DEV)
    with torch.inference_mode():
        read, _ = m.tokenizer.read(m(x))
    labels = [(m.charset_adapter(s) if i % 2 else m.charset_adapter(s)[::-1]) or 'x' for i, s in enumerate(read)]
    greedy, beam = Evaluator(m), BeamEvaluator(m, beam_width=1)
    greedy.update(x, labels)
    beam.update(x, labels)
    a, b = greedy.result(), beam.result()
    print(a, b)
    assert (a.num_samples, a.correct, a.label_length) == (b.num_samples, b.correct, b.label_length_sum)
    assert greedy.per_sample().tolist() == beam.per_sample()[:, :4].tolist() == beam.per_hypothesis().reshape(-1, 4).tolist()
    assert close(b.confidence_sum, a.confidence, 1e-5) and close(b.ned_sum, a.ned, 1e-12)


def test_host_path_model_gives_the_same_totals():
    """A train charset with 'ß' under an upper-case test charset: the table cannot say 'SS', the evaluator takes the host path."""
    from oracle.synth import charset_config, synth_state_dict
    from parseq_amd import create_model
    from parseq_amd.evaluate import BeamEvaluator
    train = CHARSET_94_FULL[:62] + 'ß'
    cfg = charset_config(CONFIGS['parseq-tiny'], train)
    model = create_model('parseq-tiny', charset_train=train, charset_test='0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ', precision='fp32')
    model.model.load_state_dict(synth_state_dict(cfg, 0))
    model = model.eval().to(DEV)
    images = synth_images(3 * (WIDTH + 1), cfg, seed=31).to(DEV)
    labels = own_nbest_labels(model, images, WIDTH)
    ev = BeamEvaluator(model, beam_width=WIDTH)
    assert ev.host_path
    ev.update(images, labels)
    with torch.inference_mode():
        result = model.beam_search(images, WIDTH)
    want = check_evaluator(ev, model, images, labels, result, WIDTH)
    assert R.coverage_holds(want, WIDTH), (want['totals'], want['first_hit'])


def test_the_searches_refusals_pass_through():
    from parseq_amd.evaluate import BeamEvaluator
    model = make_model('parseq-tiny', 'fp32')
    images = synth_images(2, CONFIGS['parseq-tiny'], seed=1).to(DEV)
    for kwargs, match in ((dict(beam_width=17), 'beam_width'), (dict(refine='score', refine_iters=2), 'refine'), (dict(alpha=0.5), 'alpha'),
                          (dict(refine='nonsense'), 'refine')):
        ev = BeamEvaluator(model, **kwargs)
        with pytest.raises(ValueError, match=match):
            ev.update(images, ['a', 'b'])
        assert ev.result().num_samples == 0
    with pytest.raises(ValueError, match='labels'):
        BeamEvaluator(model).update(images, ['a'])
    with pytest.raises(ValueError, match='lexicon'):
        BeamEvaluator(model, match=4)
    with pytest.raises(ValueError, match='256'):
        BeamEvaluator(model).update(images, ['a', 'x' * 257])


# -------------------------------------------------------------------------------------------------------------------
# test.py and tools/tune_fusion.py
# -------------------------------------------------------------------------------------------------------------------
def load_script(name, path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, path))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
    """A dozen random crops under <root>/synthetic with labels from PARSeq-Ti's own N-best (W = 3), a checkpoint of its weights, a word list."""
    from PIL import Image
    from parseq_amd.preprocess import resize_batch
    root = tmp_path_factory.mktemp('beam_eval')
    d = root / 'data' / 'synthetic'
    d.mkdir(parents=True)
    model = make_model('parseq-tiny', 'fp32')
    rng = np.random.default_rng(8)
    files = []
    for i in range(12):
        h, w = int(rng.integers(20, 60)), int(rng.integers(60, 200))
        Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(d / f'{i:02d}.png')
        files.append(str(d / f'{i:02d}.png'))
    cli = load_script('parseq_test_cli_beam', 'test.py')
    images = resize_batch(cli.load_crops(files, DEV), tuple(model.hparams.img_size))
    labels = own_nbest_labels(model, images, 3)
    (d / 'gt.txt').write_text(''.join(f'{i:02d}.png {label}\n' for i, label in enumerate(labels)), encoding='utf-8')
    ckpt = root / 'parseq-tiny.ckpt'
    torch.save({'state_dict': {k: v.cpu() for k, v in model.state_dict().items()}, 'hyper_parameters': dict(model.hparams)}, ckpt)
    words = root / 'words.txt'
    words.write_text(''.join(f'{w} {1 + i % 5}\n' for i, w in enumerate(sorted(set(labels)) + ['zebra', 'quartz'])), encoding='utf-8')
    return dict(root=str(root / 'data'), ckpt=str(ckpt), words=str(words), files=files, labels=labels, images=images)


CHARSET_TEST = '0123456789abcdefghijklmnopqrstuvwxyz'


def by_hand(cli, dataset, batch_size, **search):
    """The row test.py must print for the dataset: a `BeamEvaluator` over the batches it forms, on the checkpoint it loads."""
    from parseq_amd import load_from_checkpoint
    from parseq_amd.evaluate import BeamEvaluator
    model = load_from_checkpoint(dataset['ckpt'], charset_test=CHARSET_TEST, precision='fp32').eval().to(DEV)
    if 'words' in search:
        from parseq_amd.lexicon import Lexicon
        from parseq_amd.search_flags import load_word_list
        search['lexicon'] = Lexicon(load_word_list(search.pop('words')), model.tokenizer, fold_case=True, max_label_length=model.model.max_label_length).to(DEV)
    if 'counts' in search:
        from parseq_amd.automaton import Automaton
        from parseq_amd.search_flags import load_word_counts
        search['automaton'] = Automaton.from_lexicon(*load_word_counts(search.pop('counts')), model.tokenizer, fold_case=True).to(DEV)
    ev = BeamEvaluator(model, **search)
    for at in range(0, 12, batch_size):
        ev.update(dataset['images'][at:at + batch_size], dataset['labels'][at:at + batch_size])
    return ev.result()


@pytest.mark.parametrize('lexicon', [False, True])
def test_cli_prints_the_extended_table(lexicon, dataset, capsys, tmp_path):
    import io
    cli = load_script('parseq_test_cli_beam', 'test.py')
    plain = tmp_path / 'plain.txt'
    plain.write_text(''.join(line.split()[0] + '\n' for line in open(dataset['words'], encoding='utf-8')), encoding='utf-8')
    flags = ['--lexicon', str(plain)] if lexicon else []
    results = cli.main([dataset['ckpt'], '--data_root', dataset['root'], '--batch_size', '5', '--beam', '3', 'precision:str=fp32'] + flags)
    printed = capsys.readouterr().out
    r = by_hand(cli, dataset, 5, beam_width=3, **({'words': str(plain)} if lexicon else {}))
    want = cli.BeamTableResult('synthetic', 12, 100 * r.accuracy, 100 * (1 - r.ned), 100 * r.confidence, r.label_length, 100 * r.hit_at(3), 100 * (1 - r.oracle_ned), r.mrr)
    assert results == [want] and r.num_samples == 12
    if not lexicon:
        assert 0 < r.correct < 12 and r.hit_at(3) > r.accuracy and 0 < r.miss          # the labels stand at every rank, and nowhere
    table = io.StringIO()
    cli.print_beam_results_table([want], 3, table)
    assert table.getvalue() in printed and 'Hit@3' in printed and 'Oracle 1 - NED' in printed and 'MRR' in printed
    assert open(dataset['ckpt'] + '.log.txt').read() == table.getvalue()


def test_cli_without_flags_prints_the_greedy_table(dataset, capsys):
    import io
    from parseq_amd import load_from_checkpoint
    from parseq_amd.evaluate import Evaluator
    cli = load_script('parseq_test_cli_beam', 'test.py')
    results = cli.main([dataset['ckpt'], '--data_root', dataset['root'], '--batch_size', '5', 'precision:str=fp32'])
    printed = capsys.readouterr().out
    model = load_from_checkpoint(dataset['ckpt'], charset_test=CHARSET_TEST, precision='fp32').eval().to(DEV)
    ev = Evaluator(model)
    for at in range(0, 12, 5):
        ev.update(dataset['images'][at:at + 5], dataset['labels'][at:at + 5])
    r = ev.result()
    want = cli.Result('synthetic', 12, 100 * r.correct / 12, 100 * (1 - r.ned / 12), 100 * r.confidence / 12, r.label_length / 12)
    assert results == [want] and type(results[0]) is cli.Result
    table = io.StringIO()
    cli.print_results_table([want], table)
    kwargs = "{'precision': 'fp32', 'charset_test': '" + CHARSET_TEST + "'}"
    assert printed == f'Additional keyword arguments: {kwargs}\n' + table.getvalue()
    assert open(dataset['ckpt'] + '.log.txt').read() == table.getvalue() and 'Hit@' not in printed


def test_tuner_reports_each_grid_point_and_chooses_by_the_tie_rule(dataset, capsys, tmp_path):
    import json
    cli = load_script('parseq_test_cli_beam', 'test.py')
    tuner = load_script('parseq_tune_fusion', 'tools/tune_fusion.py')
    out = tmp_path / 'grid.json'
    grid, best = tuner.main([dataset['ckpt'], '--data_root', dataset['root'], '--batch_size', '5', '--lexicon', dataset['words'], '--priors', '--beam', '3',
                             '--alphas', '0:1:2', '--betas', '0:0.5:2', '--out', str(out), 'precision:str=fp32'])
    printed = capsys.readouterr().out
    assert [(p['alpha'], p['beta']) for p in grid] == [(0.0, 0.0), (0.0, 0.5), (1.0, 0.0), (1.0, 0.5)]
    for p in grid:
        r = by_hand(cli, dataset, 5, beam_width=3, counts=dataset['words'], alpha=p['alpha'], beta=p['beta'])
        assert (p['num_samples'], p['accuracy'], p['ned'], p['mrr']) == (12, 100 * r.accuracy, 100 * (1 - r.ned), r.mrr)
        assert p['hit'] == 100 * r.hit_at(3) and p['oracle_ned'] == 100 * (1 - r.oracle_ned)
    ranked = sorted(grid, key=lambda p: (-p['accuracy'], -p['ned'], p['alpha'], p['beta']))
    assert best == ranked[0] and json.load(open(out))['best'] == best and json.load(open(out))['grid'] == grid
    assert f'--lm-weight {best["alpha"]:g} --char-bonus {best["beta"]:g}' in printed
    # the tie rule itself, on a grid with ties at every level
    pts = [dict(alpha=a, beta=b, accuracy=acc, ned=ned) for a, b, acc, ned in ((1.0, 0.0, 50.0, 70.0), (0.5, 0.5, 50.0, 70.0), (0.5, 0.0, 50.0, 70.0),
                                                                                (0.0, 0.0, 50.0, 60.0), (0.0, 0.5, 40.0, 99.0))]
    assert tuner.choose(pts) == pts[2]
