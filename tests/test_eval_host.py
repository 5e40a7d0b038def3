"""CPU tests of the evaluation path's host side (parseq_amd/evaluate.py, test.py): the table form of CharsetAdapter, the ground-truth
encoding, the golden fixture's own consistency, gt.txt parsing and label filtering, the results table, and the cross-rank sum."""
import importlib.util
import io
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle.synth import CHARSET_36, CHARSET_200
from parseq_amd.configs import CHARSET_94_FULL
from parseq_amd.system import BatchResult, edit_distance
from parseq_amd.tokenizer import CharsetAdapter, Tokenizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHARSET_174 = CHARSET_36 + CHARSET_200[62:]
PAIRS = [(CHARSET_94_FULL, CHARSET_36), (CHARSET_94_FULL, CHARSET_94_FULL), (CHARSET_36, CHARSET_36), (CHARSET_200, CHARSET_174),
         (CHARSET_94_FULL, CHARSET_36.upper()), (CHARSET_200, CHARSET_200)]


def load_cli():
    """The repository's test.py as a module (its name shadows the standard library's `test` package, so it is loaded by path)."""
    spec = importlib.util.spec_from_file_location('parseq_test_cli', os.path.join(ROOT, 'test.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize('train,test', PAIRS)
def test_adapter_table_equals_the_adapter_per_character(train, test):
    from parseq_amd.evaluate import adapter_table
    tok, adapter = Tokenizer(train), CharsetAdapter(test)
    table = adapter_table(tok, adapter)
    assert table is not None and table.dtype == np.int32 and table.shape == (len(tok) - 2,)
    assert table[tok.eos_id] == -1
    for ch in train:
        want = adapter(ch)
        assert len(want) <= 1
        assert table[tok._stoi[ch]] == (ord(want) if want else -1), ch
    # and a string goes through the table as it goes through the adapter
    rng = np.random.default_rng(0)
    for _ in range(50):
        s = ''.join(train[i] for i in rng.integers(len(train), size=20))
        via_table = ''.join(chr(table[tok._stoi[c]]) for c in s if table[tok._stoi[c]] >= 0)
        assert via_table == adapter(s)


@pytest.mark.parametrize('train,test', [
    ('abcß', 'ABCS'),            # 'ß'.upper() == 'SS'
    ('abcİ', 'abci'),            # 'İ'.lower() is 'i' + a combining dot
    ('αβσΣ', 'αβσς'),            # str.lower() turns a word-final 'Σ' into 'ς', elsewhere into 'σ'
])
def test_charsets_a_table_cannot_express_select_the_host_path(train, test):
    from parseq_amd.evaluate import adapter_table
    assert adapter_table(Tokenizer(train), CharsetAdapter(test)) is None
    # the same characters are fine when the adapter does not fold case
    assert adapter_table(Tokenizer(train), CharsetAdapter(train + train.upper() + train.lower())) is not None


def test_evaluator_refuses_a_model_on_the_cpu():
    from parseq_amd import create_model
    from parseq_amd.evaluate import Evaluator
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        Evaluator(create_model('parseq-tiny'))


def test_ground_truth_encoding_round_trips():
    from parseq_amd.evaluate import MAX_GT, decode_ground_truth, encode_ground_truth
    labels = ['hello', '', 'a', '丘丸买', 'x\U0001F600y\U00020000', 'q' * MAX_GT]
    enc = encode_ground_truth(labels)
    n = len(labels)
    assert enc.dtype == np.int32 and enc.shape == (n + n * MAX_GT,)
    assert enc[:n].tolist() == [5, 0, 1, 3, 4, MAX_GT]
    assert enc[n + 4 * MAX_GT: n + 4 * MAX_GT + 4].tolist() == [ord('x'), 0x1F600, ord('y'), 0x20000]      # non-BMP: one code point each
    assert decode_ground_truth(enc, n) == labels
    assert encode_ground_truth(['', '']).shape == (4,)                      # width is at least 1
    assert encode_ground_truth([]).shape == (0,)
    with pytest.raises(ValueError, match=str(MAX_GT)):
        encode_ground_truth(['ok', 'q' * (MAX_GT + 1)])


def test_golden_totals_equal_the_eval_step_arithmetic():
    """The fixture minted from the reference's `_eval_step` agrees with this repository's adapter, edit distance and sums."""
    with open(os.path.join(ROOT, 'tests', 'golden', 'eval_metrics.json'), encoding='utf-8') as f:
        meta = json.load(f)
    assert len(meta['cases']) == 4
    for name, case in meta['cases'].items():
        adapter = CharsetAdapter(case['charset_test'])
        assert 16 <= len(case['labels']) <= 64
        correct = label_length = 0
        ned = confidence = 0.0
        for pred, conf, gt, dist_ in zip(case['preds'], case['row_confidence'], case['labels'], case['row_distance']):
            pred = adapter(pred)
            assert pred or gt
            assert edit_distance(pred, gt) == dist_
            confidence += conf
            ned += dist_ / max(len(pred), len(gt), 1)
            correct += int(pred == gt)
            label_length += len(pred)
        want = case['result']
        assert (want['num_samples'], want['correct'], want['label_length']) == (len(case['labels']), correct, label_length), name
        assert ned == pytest.approx(want['ned'], rel=1e-12) and confidence == pytest.approx(want['confidence'], rel=1e-12), name


def test_gt_lines_and_label_filter(tmp_path):
    cli = load_cli()
    assert cli.parse_gt_line('img/1.png Hello\n') == ('img/1.png', 'Hello')
    assert cli.parse_gt_line('img/2.png\ttwo words  here \n') == ('img/2.png', 'two words  here')
    assert cli.parse_gt_line('lonely.png\n') is None and cli.parse_gt_line('\n') is None
    lower, cased = CharsetAdapter(CHARSET_36), CharsetAdapter(CHARSET_94_FULL)
    assert cli.preprocess_label('Hello World!', lower, 25) == 'helloworld'
    assert cli.preprocess_label('Hello World!', cased, 25) == 'HelloWorld!'
    assert cli.preprocess_label('Café', lower, 25) == 'cafe'                     # NFKD, then ASCII: the accent goes
    assert cli.preprocess_label('ﬁne', lower, 25) == 'fine'                       # compatibility ligature
    assert cli.preprocess_label('!?!', lower, 25) is None                         # nothing left
    assert cli.preprocess_label('丘丸', lower, 25) is None                        # not ASCII
    assert cli.preprocess_label('a' * 26, lower, 25) is None                      # too long
    assert cli.preprocess_label('a!' * 13, lower, 25) is None                     # measured BEFORE the adapter drops characters
    assert cli.preprocess_label('a b c', lower, 3) == 'abc'                       # ... but after the whitespace is gone
    d = tmp_path / 'setA'
    d.mkdir()
    (d / 'gt.txt').write_text('1.png Hello\n2.png !!!\n\n3.png two words\n', encoding='utf-8')
    (tmp_path / 'not_a_set').mkdir()
    assert cli.find_datasets(str(tmp_path)) == ['setA']
    assert cli.read_dataset(str(tmp_path), 'setA', CHARSET_36, 25) == [(str(d / '1.png'), 'hello'), (str(d / '3.png'), 'twowords')]


def test_results_table_literal():
    cli = load_cli()
    out = io.StringIO()
    cli.print_results_table([cli.Result('IIIT5k', 3000, 99.1, 99.63, 98.127, 5.0), cli.Result('SVT', 647, 97.5, 99.2, 96.0, 5.874)], out)
    assert out.getvalue() == (
        '| Dataset  | # samples | Accuracy | 1 - NED | Confidence | Label Length |\n'
        '|:--------:|----------:|---------:|--------:|-----------:|-------------:|\n'
        '| IIIT5k   |      3000 |    99.10 |   99.63 |      98.13 |         5.00 |\n'
        '| SVT      |       647 |    97.50 |   99.20 |      96.00 |         5.87 |\n'
        '|----------|-----------|----------|---------|------------|--------------|\n'
        '| Combined |      3647 |    98.82 |   99.55 |      97.75 |         5.16 |\n')
    wide = io.StringIO()
    cli.print_results_table([cli.Result('a_long_dataset_name', 1, 100.0, 100.0, 50.0, 7.0)], wide)
    lines = wide.getvalue().splitlines()
    assert lines[0].startswith('| Dataset             | # samples |') and len({len(ln) for ln in lines}) == 1


def _free_port():
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        return sk.getsockname()[1]


def _reduce_worker(rank, world, port, q):
    os.environ['MASTER_ADDR'], os.environ['MASTER_PORT'] = '127.0.0.1', str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from parseq_amd.evaluate import reduce_result
        mine = [BatchResult(10, 7, 1.25, 8.5, 52, torch.tensor(0.5), 60), BatchResult(6, 6, 0.0, 5.75, 30, torch.tensor(2.0), 20)][rank]
        r = reduce_result(mine)
        plain = reduce_result(BatchResult(mine.num_samples, mine.correct, mine.ned, mine.confidence, mine.label_length, None, None))
        q.put((rank, (r.num_samples, r.correct, r.ned, r.confidence, r.label_length, float(r.loss), r.loss_numel),
               (plain.num_samples, plain.ned, plain.loss, plain.loss_numel)))
    finally:
        dist.destroy_process_group()


def test_two_rank_gloo_reduce():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_reduce_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for _, totals, plain in got:
        assert totals == (16, 13, 1.25, 14.25, 82, (0.5 * 60 + 2.0 * 20) / 80, 80)
        assert plain == (16, 1.25, None, None)
