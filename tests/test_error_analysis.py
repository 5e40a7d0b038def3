"""GPU tests of the error analysis: `parseq_eval_errors` (csrc/eval_errors.h) against the CPU restatement
(tests/error_analysis_reference.py) — scripts, script lengths, rows and every table, exactly —, its agreement with `parseq_eval_metrics`,
accumulation over calls and streams, every refusal, `Evaluator(errors=ErrorAnalysis)` and `test.py --analyse`."""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import error_analysis_reference as R
from gpu_util import DEV, make_model, native
from oracle.synth import CONFIGS, synth_images
from parseq_amd.configs import CHARSET_94_FULL
from parseq_amd.tokenizer import CharsetAdapter, Tokenizer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE_LENGTHS = (0, 1, 25, 31, 32, 33, 63, 64, 65, 255, 256)      # the 64-lane chunk borders of the recurrence and the array width
OTHER_BASE = 5000                                                # label code points no adapter table here produces


def adapter(kind, classes):
    """int32 [classes] with class 0 as <eos> (dropped, as `adapter_table` has it): 'identity' keeps every class apart, 'lower' folds the
    upper half of the classes onto the lower, 'drop' is the identity with every seventh class dropped."""
    table = 1000 + np.arange(classes, dtype=np.int32)
    if kind == 'lower':
        half = (classes + 1) // 2
        table[half:] = table[1:1 + classes - half]
    elif kind == 'drop':
        table[5::7] = -1
    table[0] = -1
    return table


def make_rows(L, classes, table, G, total, seed):
    """`total` rows (ids [L], length, gt [G], gt_len) — first every edge case the kernel has a path for, then short random pairs."""
    rng = np.random.default_rng(seed)
    kept = [i for i in range(1, classes) if table[i] >= 0]
    dropped = [i for i in range(classes) if table[i] < 0]
    symbols = R.symbol_set(table)
    rows = []

    def gt_row(points):
        row = rng.choice(symbols, size=G).astype(np.int32)                 # the padding is defined: a length above the width reads it
        row[:len(points)] = points[:G]
        return row

    def add(ids, points, length=None, gt_len=None):
        row = rng.integers(0, classes, size=L).astype(np.int32)             # what lies past the length must not matter
        row[:len(ids)] = ids[:L]
        rows.append((row, min(len(ids), L) if length is None else length, gt_row(list(points)), min(len(points), G) if gt_len is None else gt_len))

    def ids_near(points):
        """ids whose adapted form is `points` (those the table can produce) after a few edits."""
        back = {int(table[i]): i for i in reversed(kept)}
        ids = [back[c] for c in points if c in back]
        for _ in range(int(rng.integers(0, 4))):
            at = int(rng.integers(len(ids) + 1))
            what = int(rng.integers(3))
            if what == 0 and ids:
                ids[min(at, len(ids) - 1)] = int(rng.choice(kept))
            elif what == 1:
                ids.insert(at, int(rng.choice(kept)))
            elif ids:
                del ids[min(at, len(ids) - 1)]
        return ids

    def random_points(n, other=0.0):
        return [int(OTHER_BASE + rng.integers(50)) if rng.random() < other else int(rng.choice(symbols[:6])) for _ in range(n)]

    a, b2 = kept[0], kept[1]
    ca, cb = int(table[a]), int(table[b2])
    for n in [n for n in EDGE_LENGTHS if n <= G][::-1]:                    # the longest label first: it is in the batch of one
        points = random_points(n, other=0.1)
        add(ids_near(points), points)
        add([int(rng.choice(kept)) for _ in range(L)], random_points(n))             # a prediction of length L, no <eos>
        add([], random_points(n))                                                        # an empty prediction: n deletions
        add([a] * L, [ca] * n)                                                           # runs of one character on both sides: the tie rule
        add([a] * min(L, 3) + [b2], [ca] * n + [cb])
    equal = [int(rng.choice(kept)) for _ in range(min(L, G))]
    add(equal, [int(table[i]) for i in equal])                                           # equal strings
    add([a, b2, a][:L], [ca, cb, ca][:G])
    add([int(rng.choice(kept)) for _ in range(L)], [OTHER_BASE + k for k in range(min(G, 40))])      # no common character, label outside the symbols
    add([a] * L, [cb] * min(G, 7))                                                       # no common character, inside the symbols
    add([], [])
    add([dropped[k % len(dropped)] for k in range(L)], random_points(min(G, 4)))         # only dropped ids
    add([-3, classes, a, classes + 100, 1 << 30, b2, -1][:L], [ca, cb][:G])              # ids outside [0, C)
    add([a, dropped[0], b2, dropped[-1], a][:L], [ca, cb, ca][:G])
    for length, gt_len in ((-5, 2), (L + 9, 3), (2, -2), (1, G + 50), (-1, -1), (L + 1, G + 1)):      # the clamps
        add([int(rng.choice(kept)) for _ in range(L)], random_points(G), length=length, gt_len=gt_len)
    assert len(rows) <= total
    while len(rows) < total:
        points = random_points(int(rng.integers(0, min(G, 12) + 1)), other=0.05)
        add(ids_near(points), points)
    return rows


class Case:
    """The rows of one (L, C, table, G) and the restatement's answer for every batch size asked for (computed once)."""

    def __init__(self, L, classes, kind, G, total=260, seed=0):
        self.L, self.classes, self.G, self.table = L, classes, G, adapter(kind, classes)
        self.symbols = R.symbol_set(self.table)
        rows = make_rows(L, classes, self.table, G, total, seed)
        self.ids = np.stack([r[0] for r in rows])
        self.lengths = np.array([r[1] for r in rows], dtype=np.int32)
        self.gt = np.stack([r[2] for r in rows])
        self.gt_len = np.array([r[3] for r in rows], dtype=np.int32)
        self.preds = [R.adapt(self.ids[b], self.lengths[b], L, classes, self.table) for b in range(total)]
        self.labels = [self.gt[b, :min(max(int(self.gt_len[b]), 0), G)].tolist() for b in range(total)]
        self._want = {}

    def want(self, lo, hi):
        if (lo, hi) not in self._want:
            self._want[lo, hi] = R.analyse(self.preds[lo:hi], self.labels[lo:hi], self.symbols)
        return self._want[lo, hi]


_CASES = {}


def case(L, classes, kind, G):
    key = (L, classes, kind, G)
    if key not in _CASES:
        _CASES[key] = Case(L, classes, kind, G, seed=len(_CASES))
    return _CASES[key]


def accum_words(num_symbols):
    return R.CONFUSION + (num_symbols + 2) ** 2


def run_errors(c, lo, hi, acc=None):
    """`parseq_eval_errors` on rows lo .. hi of case `c`, on the current stream.  Returns (scripts, script_len, rows, accumulator) on the device."""
    nat, lib = native()
    n = hi - lo
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
    ids, lengths, gt, gt_len = dev(c.ids[lo:hi]), dev(c.lengths[lo:hi]), dev(c.gt[lo:hi]), dev(c.gt_len[lo:hi])
    table, symbols = dev(c.table), dev(np.array(c.symbols, dtype=np.int32))
    scripts = torch.full((n, R.SCRIPT_WIDTH), 77, dtype=torch.int8, device=DEV)
    script_len = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    rows = torch.full((n, 4), -7, dtype=torch.int32, device=DEV)
    if acc is None:
        acc = torch.zeros(accum_words(len(c.symbols)), dtype=torch.int64, device=DEV)
    assert lib.parseq_eval_errors_accum_bytes(len(c.symbols)) == 8 * acc.numel()
    nat.check(lib.parseq_eval_errors(nat.ptr(ids), nat.ptr(lengths), n, c.L, c.classes, nat.ptr(table), nat.ptr(symbols), len(c.symbols), nat.ptr(gt),
                                     nat.ptr(gt_len), c.G, nat.ptr(scripts), nat.ptr(script_len), nat.ptr(rows), nat.ptr(acc), nat.stream_ptr(ids)))
    return scripts, script_len, rows, acc


def assert_equals_restatement(got, want, tag):
    scripts, script_len, rows, acc = (t.cpu().numpy() for t in got)
    assert np.array_equal(rows, want['rows']), (tag, np.nonzero((rows != want['rows']).any(1))[0][:5])
    assert np.array_equal(script_len, want['script_len']), tag
    bad = np.nonzero((scripts != want['scripts']).any(1))[0]
    assert bad.size == 0, (tag, bad[:5], scripts[bad[0], :12], want['scripts'][bad[0], :12])
    for name, at, end in (('head', R.HEAD, R.BY_LENGTH), ('by_length', R.BY_LENGTH, R.BY_POSITION), ('by_position', R.BY_POSITION, R.CONFUSION),
                          ('confusion', R.CONFUSION, acc.size)):
        assert np.array_equal(acc[at:end], want['words'][at:end]), (tag, name)


COMBOS = [(1, 37, 'identity', 65), (7, 95, 'lower', 256), (26, 95, 'drop', 256), (32, 201, 'drop', 256), (32, 37, 'identity', 1), (26, 201, 'lower', 64),
          (7, 37, 'drop', 33)]


@pytest.mark.parametrize('L,classes,kind,G', COMBOS)
def test_operator_equals_the_restatement(L, classes, kind, G):
    """Batches of 1, 3 and 5 (a workgroup's idle waves) and 260 (more than one workgroup, the last one ragged)."""
    c = case(L, classes, kind, G)
    got = [(B, run_errors(c, 0, B)) for B in (1, 3, 5, 260)]
    torch.cuda.synchronize()
    for B, out in got:
        want = c.want(0, B)
        assert_equals_restatement(out, want, (L, classes, kind, G, B))
        R.check_identities(want['head'], want['by_length'], want['by_position'], want['confusion'], c.preds[:B], c.labels[:B])
    whole = c.want(0, 260)
    assert whole['head'][1] > 0 and whole['head'][2] > 0 and whole['head'][3] > 0 and whole['head'][4] > 0 and whole['head'][5] > 0
    if G >= 40:
        assert whole['confusion'][len(c.symbols)].sum() > 0 and whole['by_position'][32].sum() > 0      # "other" labels, positions past 31


def _near_labels(preds, rng, charset, limit=25):
    """Labels near the adapted readings `preds`: some equal, some edited, so that every operation occurs."""
    labels = []
    for p in preds:
        s = list(p)[:limit] or ['a']
        if rng.random() < 0.5:
            s[int(rng.integers(len(s)))] = charset[int(rng.integers(len(charset)))]
        if rng.random() < 0.3 and len(s) > 1:
            del s[int(rng.integers(len(s)))]
        if rng.random() < 0.3:
            s.insert(int(rng.integers(len(s) + 1)), charset[int(rng.integers(len(charset)))])
        labels.append(''.join(s))
    return labels


def test_rows_equal_the_metrics_entry():
    """`rows_out` of the two entries on the same logits: the error analysis starts from the ids and lengths the metrics entry wrote."""
    from parseq_amd.evaluate import adapter_table, encode_ground_truth, symbol_table
    nat, lib = native()
    tok = Tokenizer(CHARSET_94_FULL)
    table = adapter_table(tok, CharsetAdapter(CHARSET_94_FULL[:36]))
    symbols = symbol_table(table)
    assert len(symbols) == 36
    rng = np.random.default_rng(11)
    n, length, classes = 70, 26, len(tok) - 2
    strings = [''.join(CHARSET_94_FULL[k] for k in rng.integers(94, size=int(rng.integers(0, 26)))) for _ in range(n)]
    labels = _near_labels([CharsetAdapter(CHARSET_94_FULL[:36])(s) for s in strings], rng, CHARSET_94_FULL[:36])
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(n, length, classes, generator=g)
    for r, s in enumerate(strings):
        for pos, i in enumerate(tok._tok2ids(s) + ([tok.eos_id] if len(s) < length else [])):
            logits[r, pos, i] = 9.0
    logits = logits.to(DEV)
    enc = torch.from_numpy(encode_ground_truth(labels)).to(DEV)
    width = (enc.numel() - n) // n
    ids = torch.empty((n, length), dtype=torch.int32, device=DEV)
    lengths = torch.empty((n,), dtype=torch.int32, device=DEV)
    conf = torch.empty((n,), dtype=torch.float32, device=DEV)
    rows = torch.empty((n, 4), dtype=torch.int32, device=DEV)
    ws = torch.empty(n, dtype=torch.float64, device=DEV)
    totals = torch.zeros(5, dtype=torch.int64, device=DEV)
    d_table, d_symbols = torch.from_numpy(table).to(DEV), torch.from_numpy(symbols).to(DEV)
    nat.check(lib.parseq_eval_metrics(nat.ptr(logits), n, length, classes, tok.eos_id, nat.ptr(d_table), nat.ptr(enc[n:]), nat.ptr(enc), width, nat.ptr(ids),
                                      nat.ptr(lengths), nat.ptr(conf), nat.ptr(rows), nat.ptr(ws), nat.ptr(totals), nat.stream_ptr(logits)))
    scripts = torch.empty((n, R.SCRIPT_WIDTH), dtype=torch.int8, device=DEV)
    script_len = torch.empty((n,), dtype=torch.int32, device=DEV)
    rows2 = torch.full((n, 4), -7, dtype=torch.int32, device=DEV)
    acc = torch.zeros(accum_words(36), dtype=torch.int64, device=DEV)
    nat.check(lib.parseq_eval_errors(nat.ptr(ids), nat.ptr(lengths), n, length, classes, nat.ptr(d_table), nat.ptr(d_symbols), 36, nat.ptr(enc[n:]), nat.ptr(enc),
                                     width, nat.ptr(scripts), nat.ptr(script_len), nat.ptr(rows2), nat.ptr(acc), nat.stream_ptr(logits)))
    torch.cuda.synchronize()
    assert torch.equal(rows2.cpu(), rows.cpu()) and 0 < int(rows[:, 3].sum()) < n
    samples, correct, label_length = totals[:3].tolist()
    head = acc[:8].tolist()
    assert (head[0], head[5], head[1] + head[2] + head[3]) == (samples, correct, label_length)
    preds = [[ord(ch) for ch in CharsetAdapter(CHARSET_94_FULL[:36])(s)] for s in strings]
    want = R.analyse(preds, [[ord(ch) for ch in y] for y in labels], symbols.tolist())
    assert_equals_restatement((scripts, script_len, rows2, acc), want, 'after the metrics entry')


def test_accumulation_over_calls_and_streams():
    c = case(26, 95, 'drop', 256)
    want = c.want(0, 260)                                       # rows 0 .. 200 and 200 .. 260 into one accumulator = the whole batch
    first = run_errors(c, 0, 200)
    run_errors(c, 200, 260, acc=first[3])
    torch.cuda.synchronize()
    assert np.array_equal(first[3].cpu().numpy(), want['words'])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = run_errors(c, 0, 200)
        run_errors(c, 200, 260, acc=other[3])
    side.synchronize()
    assert torch.equal(other[3].cpu(), first[3].cpu())
    again = run_errors(c, 0, 200)
    run_errors(c, 200, 260, acc=again[3])
    torch.cuda.synchronize()
    assert torch.equal(again[3].cpu(), first[3].cpu())
    for k in range(3):
        assert torch.equal(again[k].cpu(), first[k].cpu()) and torch.equal(other[k].cpu(), first[k].cpu())


def test_refusals_leave_outputs_and_accumulator_untouched():
    nat, lib = native()
    n, L, classes, G, T = 4, 8, 37, 16, 36
    table = torch.from_numpy(adapter('identity', classes)).to(DEV)
    symbols = torch.from_numpy(np.array(R.symbol_set(adapter('identity', classes)), dtype=np.int32)).to(DEV)
    ids = torch.ones((n, L), dtype=torch.int32, device=DEV)
    lengths = torch.full((n,), 3, dtype=torch.int32, device=DEV)
    gt = torch.full((n, 300), 1001, dtype=torch.int32, device=DEV)
    gt_len = torch.full((n,), 3, dtype=torch.int32, device=DEV)
    scripts = torch.full((n, R.SCRIPT_WIDTH), 77, dtype=torch.int8, device=DEV)
    script_len = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    rows = torch.full((n, 4), -7, dtype=torch.int32, device=DEV)
    acc = torch.full((accum_words(T),), -99, dtype=torch.int64, device=DEV)
    good = dict(ids=nat.ptr(ids), lengths=nat.ptr(lengths), batch=n, L=L, C=classes, table=nat.ptr(table), symbols=nat.ptr(symbols), T=T, gt=nat.ptr(gt),
                gt_len=nat.ptr(gt_len), G=G, scripts=nat.ptr(scripts), script_len=nat.ptr(script_len), rows=nat.ptr(rows), acc=nat.ptr(acc))
    cases = [({k: C.c_void_p(0)}, 'null argument') for k in ('ids', 'lengths', 'table', 'symbols', 'gt', 'gt_len', 'scripts', 'script_len', 'rows', 'acc')]
    cases += [({'batch': 0}, 'batch = 0'), ({'batch': -2}, 'batch = -2'), ({'L': 0}, 'L = 0'), ({'L': 33}, 'L = 33'), ({'C': 0}, 'C = 0'),
              ({'G': 0}, 'gt_width = 0'), ({'G': 257}, 'gt_width = 257'), ({'T': 0}, 'num_symbols = 0'), ({'T': 513}, 'num_symbols = 513')]
    for change, message in cases:
        a = dict(good, **change)
        status = lib.parseq_eval_errors(a['ids'], a['lengths'], a['batch'], a['L'], a['C'], a['table'], a['symbols'], a['T'], a['gt'], a['gt_len'], a['G'],
                                        a['scripts'], a['script_len'], a['rows'], a['acc'], nat.stream_ptr(ids))
        error = lib.parseq_last_error().decode()
        assert status == -1 and 'eval_errors' in error and message in error, (change, status, error)
    torch.cuda.synchronize()
    assert (scripts == 77).all() and (script_len == -7).all() and (rows == -7).all() and (acc == -99).all()
    assert lib.parseq_eval_errors_accum_bytes(0) == 0 and lib.parseq_eval_errors_accum_bytes(513) == 0 and lib.parseq_eval_errors_accum_bytes(-1) == 0
    assert lib.parseq_eval_errors_accum_bytes(1) == 8 * (272 + 9) and lib.parseq_eval_errors_accum_bytes(512) == 8 * (272 + 514 * 514)
    # and the unchanged arguments are accepted
    a = good
    nat.check(lib.parseq_eval_errors(a['ids'], a['lengths'], a['batch'], a['L'], a['C'], a['table'], a['symbols'], a['T'], a['gt'], a['gt_len'], a['G'],
                                     a['scripts'], a['script_len'], a['rows'], a['acc'], nat.stream_ptr(ids)))
    torch.cuda.synchronize()
    assert rows.cpu().tolist() == [[3, 3, 0, 1]] * n and int(acc[0]) == -99 + n


def _system(name):
    """(synthetic-weight system on the device, its oracle configuration); 'host-path': a charset pair no adapter table expresses."""
    if name == 'vitstr':
        from oracle import vitstr_oracle as V
        from parseq_amd import create_model
        cfg = V.vitstr_config()
        m = create_model('vitstr', precision='bf16x3')
        m.model.load_state_dict(V.synth_state_dict(cfg, 0))
        return m.eval().to(DEV), cfg
    if name == 'host-path':
        from oracle.synth import charset_config, synth_state_dict
        from parseq_amd import create_model
        train = CHARSET_94_FULL[:62] + 'ß'                      # 'ß'.upper() == 'SS'
        cfg = charset_config(CONFIGS['parseq-tiny'], train)
        m = create_model('parseq-tiny', charset_train=train, charset_test='0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ', precision='bf16x3')
        m.model.load_state_dict(synth_state_dict(cfg, 0))
        return m.eval().to(DEV), cfg
    return make_model(name, 'bf16x3'), CONFIGS[name]


@pytest.mark.parametrize('name', ['parseq-tiny', 'vitstr', 'host-path'])
def test_evaluator_with_an_error_analysis(name):
    from parseq_amd.evaluate import ErrorAnalysis, Evaluator
    model, cfg = _system(name)
    rng = np.random.default_rng(3)
    errors = ErrorAnalysis(model)
    plain, ev = Evaluator(model), Evaluator(model, errors=errors)
    assert ev.host_path == errors.host_path == plain.host_path == (name == 'host-path')
    preds_all, labels_all = [], []
    for seed, n in ((1, 16), (2, 5), (3, 33)):
        images = synth_images(n, cfg, seed=seed).to(DEV)
        with torch.inference_mode():
            preds = [model.charset_adapter(p) for p in model.tokenizer.read(model(images))[0]]
        labels = _near_labels(preds, rng, model.hparams.charset_test, model.hparams.max_label_length)
        plain.update(images, labels)
        ev.update(images, labels)
        preds_all += preds; labels_all += labels
    got, want = ev.result(), plain.result()
    assert got == want and 0 < got.correct < got.num_samples
    report = errors.result()
    assert report.symbols == sorted(report.symbols) and set(''.join(preds_all)) <= set(report.symbols)
    R.check_identities(report.head, report.by_length, report.by_position, report.confusion, preds_all, labels_all)
    assert (report.exact, report.matches + report.substitutions + report.insertions, report.samples) == (got.correct, got.label_length, got.num_samples)
    assert np.array_equal(report._words(), R.analyse(preds_all, labels_all, report.symbols)['words'])
    scripts, script_len, rows = errors.per_sample()            # the last batch
    last = R.analyse(preds_all[-33:], labels_all[-33:], report.symbols)
    assert np.array_equal(scripts, last['scripts']) and np.array_equal(script_len, last['script_len']) and np.array_equal(rows, last['rows'])
    if name != 'host-path':
        assert np.array_equal(ev.per_sample(), plain.per_sample()) and np.array_equal(rows, ev.per_sample())
    ev.reset()
    assert errors.result().samples == 0 and not errors.result().confusion.any()


def test_cli_analyse_writes_the_restatements_tables(tmp_path, monkeypatch, capsys):
    from PIL import Image
    spec = importlib.util.spec_from_file_location('parseq_test_cli', os.path.join(ROOT, 'test.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    spec = importlib.util.spec_from_file_location('parseq_read_cli', os.path.join(ROOT, 'read.py'))
    read_cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(read_cli)
    model = make_model('parseq', 'bf16x3')
    monkeypatch.setattr(cli, 'load_from_checkpoint', lambda ckpt, **kw: model)
    rng = np.random.default_rng(8)
    root = tmp_path / 'data'
    names, preds, labels = ['setA', 'setB'], {}, {}
    for name, count in zip(names, (7, 5)):
        d = root / name
        d.mkdir(parents=True)
        files = []
        for i in range(count):
            h, w = int(rng.integers(20, 60)), int(rng.integers(60, 200))
            Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(d / f'{i}.png')
            files.append(str(d / f'{i}.png'))
        read = [r for at in range(0, count, 4) for r in read_cli.read_files(model, files[at:at + 4], DEV)]      # the batches --batch_size 4 forms
        preds[name] = [model.charset_adapter(label) for _, label, _ in read]
        labels[name] = _near_labels(preds[name], rng, model.hparams.charset_test, limit=20)      # (the label filter drops labels of more than 25)
        labels[name][0], labels[name][1] = preds[name][0][:25] or 'a', preds[name][1][:20] + 'a'      # one label read exactly (unless nothing was read), one not
        (d / 'gt.txt').write_text(''.join(f'{i}.png {y}\n' for i, y in enumerate(labels[name])), encoding='utf-8')
    ckpt = str(tmp_path / 'model.ckpt')
    argv = [ckpt, '--data_root', str(root), '--batch_size', '4', '--device', DEV]
    capsys.readouterr()
    cli.main(argv)
    plain_out, plain_log = capsys.readouterr().out, open(ckpt + '.log.txt').read()
    assert not os.path.exists(ckpt + '.errors.json')
    os.remove(ckpt + '.log.txt')
    cli.main(argv + ['--analyse', '3'])
    out = capsys.readouterr().out
    assert out.startswith(plain_out) and open(ckpt + '.log.txt').read() == plain_log and plain_log in plain_out
    assert 'setA: 7 samples' in out[len(plain_out):] and 'All datasets: 12 samples' in out[len(plain_out):]
    with open(ckpt + '.errors.json', encoding='utf-8') as f:
        written = json.load(f)
    symbols = sorted(set(model.hparams.charset_test))
    assert written['top'] == 3 and list(written['datasets']) == names
    both = R.analyse(preds['setA'] + preds['setB'], labels['setA'] + labels['setB'], symbols)
    for got, want in [(written['datasets'][name], R.analyse(preds[name], labels[name], symbols)) for name in names] + [(written['combined'], both)]:
        assert got['symbols'] == symbols
        for key in ('head', 'by_length', 'by_position', 'confusion'):
            assert np.array_equal(np.array(got[key], dtype=np.int64), want[key]), key
    assert both['head'][5] == sum(p == y for name in names for p, y in zip(preds[name], labels[name])) < 12
