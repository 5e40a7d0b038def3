"""CPU tests of the error analysis: the definition itself (tests/error_analysis_reference.py), the stored-column formula
the kernel reads the table from, `host_edit_script` and the host tables against the restatement, the symbol table, `ErrorReport`'s helpers,
test.py's --analyse flag and the cross-rank sum."""
import importlib.util
import os
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

import error_analysis_reference as R
from oracle.synth import CHARSET_36, CHARSET_200
from parseq_amd.configs import CHARSET_94_FULL
from parseq_amd.system import edit_distance
from parseq_amd.tokenizer import CharsetAdapter, Tokenizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHARSET_174 = CHARSET_36 + CHARSET_200[62:]
M_SIZES = (0, 1, 2, 5, 25, 31, 32)
N_SIZES = (0, 1, 3, 25, 33, 64, 65, 100, 256)
LITERALS = [('aaa', 'aa', [2, 0, 0]), ('hcllo', 'hello', [0, 1, 0, 0, 0]), ('', 'ab', [3, 3]), ('ab', '', [2, 2]), ('', '', [])]


def load_cli():
    spec = importlib.util.spec_from_file_location('parseq_test_cli', os.path.join(ROOT, 'test.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def random_pairs(alphabet, seed=0):
    """One pair of strings per (m, n) of the grid, over the first `alphabet` lower-case letters."""
    rng = np.random.default_rng(seed + alphabet)
    letters = 'abcdefgh'[:alphabet]
    return [(''.join(letters[k] for k in rng.integers(alphabet, size=m)), ''.join(letters[k] for k in rng.integers(alphabet, size=n)))
            for m in M_SIZES for n in N_SIZES]


@pytest.fixture(scope='module')
def pairs():
    return {alphabet: random_pairs(alphabet) for alphabet in (2, 3, 8)}


@pytest.mark.parametrize('alphabet', [2, 3, 8])
def test_the_script_of_the_definition_is_an_optimal_alignment(alphabet, pairs):
    for p, g in pairs[alphabet]:
        script = R.edit_script(p, g)
        cost, pred_side, label_side, applied = R.replay(script, p, g)
        assert cost == edit_distance(p, g), (p, g)
        assert ''.join(pred_side) == p and ''.join(label_side) == g and ''.join(applied) == g
        assert len(script) <= len(p) + len(g) <= R.SCRIPT_WIDTH


def test_literal_scripts():
    from parseq_amd.evaluate import host_edit_script
    for p, g, want in LITERALS:
        assert R.edit_script(p, g) == want, (p, g)
        assert host_edit_script(p, g) == want, (p, g)


@pytest.mark.parametrize('alphabet', [2, 3, 8])
def test_stored_columns_give_every_table_entry(alphabet, pairs):
    """D[i][j] = j + popc(Pv_j & ((1 << i) - 1)) - popc(Mv_j & ((1 << i) - 1)), also from the low 32 bits the kernel keeps."""
    checked = 0
    for p, g in pairs[alphabet] + random_pairs(alphabet, seed=7):
        if len(g) > 100:
            continue
        table, columns = R.levenshtein_table(p, g), R.myers_columns(p, g)
        assert len(columns) == len(g) + 1
        for j, column in enumerate(columns):
            low = (column[0] & 0xffffffff, column[1] & 0xffffffff)
            for i in range(len(p) + 1):
                assert R.column_entry(column, i, j) == table[i, j] == R.column_entry(low, i, j), (p, g, i, j)
        checked += 1
    assert checked >= 100


@pytest.mark.parametrize('alphabet', [2, 3, 8])
def test_host_edit_script_equals_the_restatement(alphabet, pairs):
    from parseq_amd.evaluate import host_edit_script
    for p, g in pairs[alphabet]:
        assert host_edit_script(p, g) == R.edit_script(p, g), (p, g)


@pytest.mark.parametrize('train,test,count', [(CHARSET_94_FULL, CHARSET_36, 36), (CHARSET_94_FULL, CHARSET_94_FULL, 94), (CHARSET_36, CHARSET_36, 36),
                                              (CHARSET_200, CHARSET_174, None)])
def test_symbol_table(train, test, count):
    from parseq_amd.evaluate import adapter_table, symbol_table
    table = adapter_table(Tokenizer(train), CharsetAdapter(test))
    symbols = symbol_table(table)
    assert symbols.dtype == np.int32 and symbols.tolist() == R.symbol_set(table)
    assert (np.diff(symbols) > 0).all() and symbols.min() >= 0
    adapter = CharsetAdapter(test)
    assert symbols.tolist() == sorted({ord(c) for ch in train for c in adapter(ch)})
    if count is not None:
        assert len(symbols) == count


def _random_batch(seed, symbols='abcde', foreign='xyz', rows=60):
    """Adapted predictions over `symbols` (m <= 32) and labels over `symbols` + `foreign`, near each other, of every kind of length."""
    rng = np.random.default_rng(seed)
    preds, labels = [], []
    for r in range(rows):
        n = int(rng.choice([0, 1, 3, 7, 12, 31, 32, 33, 40, 70]))
        gt = [(symbols + foreign)[k] for k in rng.integers(len(symbols) + (len(foreign) if r % 3 == 0 else 0), size=n)]
        pred = [c for c in gt if c in symbols]
        for _ in range(int(rng.integers(0, 4))):
            kind = rng.integers(3)
            at = int(rng.integers(len(pred) + 1))
            if kind == 0 and pred:
                pred[min(at, len(pred) - 1)] = symbols[int(rng.integers(len(symbols)))]
            elif kind == 1:
                pred.insert(at, symbols[int(rng.integers(len(symbols)))])
            elif pred:
                del pred[min(at, len(pred) - 1)]
        preds.append(''.join(pred[:32]))
        labels.append(''.join(gt))
    return preds, labels


@pytest.mark.parametrize('seed', [1, 2])
def test_table_identities_and_host_tables(seed):
    """The identities of section 28 hold for the restatement's tables, and `host_error_tables` gives exactly those tables."""
    from parseq_amd.evaluate import host_error_tables
    symbols = 'abcde'
    preds, labels = _random_batch(seed, symbols)
    want = R.analyse(preds, labels, symbols)
    R.check_identities(want['head'], want['by_length'], want['by_position'], want['confusion'], preds, labels)
    assert want['head'][2] > 0 and want['head'][3] > 0 and want['head'][4] > 0 and want['confusion'][len(symbols)].sum() > 0      # every kind occurs, "other" too
    assert want['by_length'][32, 0] > 0 and want['by_position'][32].sum() > 0
    got = host_error_tables(preds, labels, list(symbols))
    R.check_identities(got.head, got.by_length, got.by_position, got.confusion, preds, labels)
    assert np.array_equal(got._words(), want['words'])
    assert (got.samples, got.matches, got.substitutions, got.insertions, got.deletions, got.exact) == tuple(int(v) for v in want['head'][:6])


def _hand_made_report():
    from parseq_amd.evaluate import LEN_BINS, ErrorReport
    symbols = ['a', 'b', 'c']                                   # T = 3: index 3 is "other", 4 "none"
    confusion = np.zeros((5, 5), dtype=np.int64)
    confusion[0, 0], confusion[1, 1], confusion[2, 2] = 50, 40, 30
    confusion[0, 1] = 4; confusion[2, 0] = 4; confusion[1, 0] = 7; confusion[3, 2] = 4; confusion[1, 2] = 1      # three cells tie at 4
    confusion[0, 4] = 2; confusion[2, 4] = 2; confusion[3, 4] = 5                                                 # deletions: 'a' and 'c' tie
    confusion[4, 1] = 3; confusion[4, 0] = 3; confusion[4, 2] = 1                                                 # insertions: 'a' and 'b' tie
    by_length = np.zeros((LEN_BINS, 4), dtype=np.int64)
    by_length[3] = (10, 5, 9, 30); by_length[7] = (4, 4, 0, 28); by_length[32] = (2, 0, 11, 80)
    by_position = np.zeros((LEN_BINS, 4), dtype=np.int64)
    by_position[0] = (16, 2, 0, 1); by_position[1] = (16, 0, 4, 0); by_position[32] = (0, 0, 0, 6)
    head = np.array([16, 120, 20, 7, 9, 9, 0, 0], dtype=np.int64)
    return ErrorReport(symbols, head, by_length, by_position, confusion)


def test_report_helpers_and_json_round_trip():
    from parseq_amd.evaluate import NONE, OTHER, ErrorReport
    r = _hand_made_report()
    assert (r.samples, r.matches, r.substitutions, r.insertions, r.deletions, r.exact) == (16, 120, 20, 7, 9, 9)
    assert r.top_confusions(10) == [('b', 'a', 7), ('a', 'b', 4), ('c', 'a', 4), (OTHER, 'c', 4), ('b', 'c', 1)]      # ties by (label, predicted) index
    assert r.top_confusions(2) == [('b', 'a', 7), ('a', 'b', 4)] and r.top_confusions(0) == []
    assert r.top_deleted(5) == [(OTHER, 5), ('a', 2), ('c', 2)] and r.top_deleted(1) == [(OTHER, 5)]
    assert r.top_inserted(5) == [('a', 3), ('b', 3), ('c', 1)]
    assert r.accuracy_by_length() == [(3, 10, 0.5), (7, 4, 1.0), (32, 2, 0.0)]
    assert r.error_rate_by_position() == [(0, 16, 2 / 16, 1), (1, 16, 4 / 16, 0), (32, 0, 0.0, 6)]
    assert r.name(3) == OTHER and r.name(4) == NONE
    back = ErrorReport.from_json(r.to_json())
    assert back == r and back.confusion.dtype == np.int64 and back.symbols == r.symbols
    assert back.top_confusions(10) == r.top_confusions(10)
    both = r + back
    assert both.samples == 32 and np.array_equal(both.confusion, 2 * r.confusion) and np.array_equal(both.by_length, 2 * r.by_length)
    with pytest.raises(ValueError, match='symbol'):
        r + ErrorReport(['a', 'b', 'd'], r.head, r.by_length, r.by_position, r.confusion)


def test_error_analysis_refuses_a_model_on_the_cpu():
    from parseq_amd import create_model
    from parseq_amd.evaluate import ErrorAnalysis
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ErrorAnalysis(create_model('parseq-tiny'))


@pytest.mark.parametrize('argv,message', [
    (['ckpt', '--analyse', '--beam', '3'], 'not with a search flag'),
    (['ckpt', '--analyse', '5', '--lexicon', 'words.txt'], 'not with a search flag'),
    (['ckpt', '--analyse', '--lm', 'corpus.txt'], 'not with a search flag'),
    (['ckpt', '--analyse', '0'], 'at least 1'),
    (['ckpt', '--analyse', '-4'], 'at least 1'),
])
def test_analyse_flag_refusals(argv, message, capsys, monkeypatch):
    cli = load_cli()

    def no_model(*a, **kw):
        raise AssertionError('the model must not be loaded after an argument error')
    monkeypatch.setattr(cli, 'load_from_checkpoint', no_model)
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2                                    # parser.error, before any model is loaded
    assert message in capsys.readouterr().err


def test_analyse_flag_parsing():
    cli = load_cli()
    parser = cli.build_parser()
    before = dict(checkpoint='ckpt', data_root='data', batch_size=512, cased=False, punctuation=False, rotation=0, device='cuda', beam=None, lexicon=None,
                  priors=False, lm=None, lm_order=None, pattern=None, lm_weight=None, char_bonus=None, match=None, refine_beams=None, refine_iters=None,
                  auto_rotate=None, upright_bias=None)
    args, unknown = parser.parse_known_args(['ckpt'])
    assert vars(args) == dict(before, analyse=None) and unknown == []
    assert cli.resolve_analysis(parser, args, None) is None
    args, unknown = parser.parse_known_args(['ckpt', '--analyse', '--cased', 'refine_iters:int=2'])
    assert vars(args) == dict(before, analyse=20, cased=True) and unknown == ['refine_iters:int=2']
    assert cli.resolve_analysis(parser, args, None) == 20
    args, _ = parser.parse_known_args(['ckpt', '--rotation', '90', '--analyse', '7', '--auto-rotate', 'flip'])
    assert (args.analyse, args.rotation, args.auto_rotate) == (7, 90, 'flip') and cli.resolve_analysis(parser, args, None) == 7


def test_print_error_report_literal(capsys):
    cli = load_cli()
    cli.print_error_report('IIIT5k', _hand_made_report(), 2)
    assert capsys.readouterr().out == (
        '\nIIIT5k: 16 samples, 9 read exactly; 120 matches, 20 substitutions, 7 insertions, 9 deletions\n'
        '| Label length | # samples | Accuracy |\n'
        '|-------------:|----------:|---------:|\n'
        '|            3 |        10 |    50.00 |\n'
        '|            7 |         4 |   100.00 |\n'
        '|          32+ |         2 |     0.00 |\n'
        "Most frequent confusions (label -> read): 'b' -> 'a' x 7, 'a' -> 'b' x 4\n"
        "Most frequent deletions (label characters not read): '<other>' x 5, 'a' x 2\n"
        "Most frequent insertions (characters read that the label lacks): 'a' x 3, 'b' x 3\n")


def _free_port():
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        return sk.getsockname()[1]


def _reduce_worker(rank, world, port, q):
    os.environ['MASTER_ADDR'], os.environ['MASTER_PORT'] = '127.0.0.1', str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from parseq_amd.evaluate import host_error_tables, reduce_report
        preds, labels = _random_batch(10 + rank, rows=20 + 5 * rank)
        r = reduce_report(host_error_tables(preds, labels, list('abcde')))
        q.put((rank, r.symbols, r._words().tolist()))
    finally:
        dist.destroy_process_group()


def test_two_rank_gloo_reduce_of_reports():
    from parseq_amd.evaluate import host_error_tables
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
    parts = [host_error_tables(*_random_batch(10 + rank, rows=20 + 5 * rank), list('abcde')) for rank in range(2)]
    want = parts[0] + parts[1]
    assert want.samples == 45
    for _, symbols, words in got:
        assert symbols == list('abcde') and words == want._words().tolist()
