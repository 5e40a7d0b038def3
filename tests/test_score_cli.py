"""GPU tests of the command lines of scoring: read.py --candidates / --expect on rendered words and on the regions of a
scene, test.py --audit on a folder with two planted wrong labels, and both programs without the new flags."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from gpu_util import DEV, make_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_script(name, path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, path))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@pytest.fixture(scope='module')
def words(tmp_path_factory):
    folder = tmp_path_factory.mktemp('score_words')
    labels = _load_script('parseq_tool_make_text_dataset_score', 'tools/make_text_dataset.py').write_dataset(str(folder), 8, seed=3)
    return [str(folder / f'{i:06d}.png') for i in range(8)], labels


def _batch(cli, model, files):
    from parseq_amd.preprocess import resize_batch
    crops = [torch.from_numpy(np.asarray(cli.Image.open(f).convert('RGB')).copy()).to(DEV) for f in files]
    return resize_batch(crops, tuple(model.hparams.img_size))


def test_read_cli_candidates_and_expect(words, tmp_path, monkeypatch, capsys):
    cli = _load_script('parseq_read_cli_score', 'read.py')
    files, labels = words[0][:3], words[1][:3]
    m = make_model('parseq-tiny', 'bf16x3')
    monkeypatch.setattr(cli, 'load_from_checkpoint', lambda ckpt, **kw: m)
    batch = _batch(cli, m, files)
    with torch.inference_mode():
        readings, _ = m.tokenizer.read(m(batch))
    # without the flags: the lines of the greedy reading, nothing else
    cli.main(['pretrained=parseq-tiny', '--images', *files, '--device', DEV])
    assert capsys.readouterr().out.splitlines()[1:] == [f'{f}: {r}' for f, r in zip(files, readings)]
    # --candidates: ragged lists, an empty string among them
    cands = [[labels[0], labels[0] + 'x', 'Zq9'], [labels[1]], ['', labels[2], labels[2][::-1], 'a']]
    path = tmp_path / 'cands.txt'
    path.write_text(''.join('\t'.join(c) + '\n' for c in cands), encoding='utf-8')
    for extra, kw in (([], {}), (['--orders', 'both', '--length-norm'], dict(orders='both', normalize=True))):
        cli.main(['pretrained=parseq-tiny', '--images', *files, '--device', DEV, '--candidates', str(path)] + extra)
        printed = capsys.readouterr().out.splitlines()[1:]
        with torch.inference_mode():
            res = m.score(batch, cands, **kw)
        ranked = m.tokenizer.decode_scores(res, cands)
        want = []
        for f, alts in zip(files, ranked):
            want += [f'{f}: {alts[0][0]}'] + [f'    {s:9.4f}  {c}' for c, s, _ in alts]
        assert printed == want and [len(a) for a in ranked] == [3, 1, 4]
        rank = res.rank.cpu().tolist()
        assert [[c for c, _, _ in alts] for alts in ranked] == [[cands[b][j] for j in rank[b] if j < len(cands[b])] for b in range(3)]
    # --expect: the reading, then both scores
    cli.main(['pretrained=parseq-tiny', '--images', *files, '--device', DEV, '--expect', *labels])
    printed = capsys.readouterr().out.splitlines()[1:]
    limit = m.model.max_label_length
    pairs = [[w] + ([r] if len(r) <= limit else []) for w, r in zip(labels, readings)]
    with torch.inference_mode():
        scores = m.score(batch, pairs).scores.cpu().tolist()
    want = []
    for f, pair, row in zip(files, pairs, scores):
        want += [f'{f}: {pair[1] if len(pair) > 1 else ""}', f'    {row[0]:9.4f}  expected  {pair[0]}'] + ([f'    {row[1]:9.4f}  read      {pair[1]}'] if len(pair) > 1 else [])
    assert printed == want and all(np.isfinite(row[0]) for row in scores)
    # refusals that need the files: a count that does not match, a foreign character
    with pytest.raises(SystemExit):
        cli.main(['pretrained=parseq-tiny', '--images', *files, '--device', DEV, '--expect', 'ab'])
    with pytest.raises(SystemExit, match='charset'):
        cli.main(['pretrained=parseq-tiny', '--images', *files, '--device', DEV, '--expect', 'ab', 'cd', 'eé'])
    path.write_text('a\n', encoding='utf-8')
    with pytest.raises(SystemExit, match='one line of candidates per crop'):
        cli.main(['pretrained=parseq-tiny', '--images', *files, '--device', DEV, '--candidates', str(path)])
    capsys.readouterr()


def test_read_cli_expect_on_regions(tmp_path, monkeypatch, capsys):
    from PIL import Image
    cli = _load_script('parseq_read_cli_score_regions', 'read.py')
    rng = np.random.default_rng(5)
    scene = str(tmp_path / 'scene.png')
    Image.fromarray(rng.integers(0, 256, size=(120, 160, 3), dtype=np.uint8), 'RGB').save(scene)
    quads = [[(10, 10), (150, 14), (148, 50), (9, 44)], [(20, 60), (120, 62), (118, 100), (22, 98)]]
    rf = tmp_path / 'scene.txt'
    rf.write_text(''.join(','.join(f'{v}' for p in q for v in p) + '\n' for q in quads), encoding='utf-8')
    m = make_model('parseq-tiny', 'bf16x3')
    monkeypatch.setattr(cli, 'load_from_checkpoint', lambda ckpt, **kw: m)
    cli.main(['pretrained=parseq-tiny', '--images', scene, '--regions', str(rf), '--device', DEV, '--expect', 'stop', 'go', '--orders', 'mirrored'])
    printed = capsys.readouterr().out.splitlines()[1:]
    names, batch, _ = cli.load_region_batch(m, [scene], [str(rf)], DEV)
    assert names == [f'{scene}#0', f'{scene}#1']
    with torch.inference_mode():
        readings, _ = m.tokenizer.read(m(batch))
        scores = m.score(batch, [['stop', readings[0]], ['go', readings[1]]], orders='mirrored').scores.cpu().tolist()
    assert all(len(r) <= m.model.max_label_length for r in readings)
    want = []
    for name, w, r, row in zip(names, ('stop', 'go'), readings, scores):
        want += [f'{name}: {r}', f'    {row[0]:9.4f}  expected  {w}', f'    {row[1]:9.4f}  read      {r}']
    assert printed == want


def test_test_cli_audit(tmp_path, capsys):
    """Labels = what the model reads, but for two planted ones: the audit lists exactly those two, with the scores `score` gives the pair."""
    import shutil
    from parseq_amd import load_from_checkpoint
    cli = _load_script('parseq_test_cli_audit', 'test.py')
    charset_test = '0123456789abcdefghijklmnopqrstuvwxyz'
    model = make_model('parseq-tiny', 'fp32')
    ckpt = str(tmp_path / 'parseq-tiny.ckpt')
    torch.save({'state_dict': {k: v.cpu() for k, v in model.state_dict().items()}, 'hyper_parameters': dict(model.hparams)}, ckpt)
    model = load_from_checkpoint(ckpt, charset_test=charset_test, precision='fp32').eval().to(DEV)
    # an untrained model reads mostly what the test charset drops: render enough words that six readings survive the label filter
    pool = tmp_path / 'pool'
    _load_script('parseq_tool_make_text_dataset_audit', 'tools/make_text_dataset.py').write_dataset(str(pool), 64, seed=5)
    candidates = [str(pool / f'{i:06d}.png') for i in range(64)]
    with torch.inference_mode():
        first, _ = model.tokenizer.read(model(_batch(cli, model, candidates)))
    kept = [f for f, r in zip(candidates, first) if 0 < len(model.charset_adapter(r)) and len(r) <= model.hparams.max_label_length][:6]
    assert len(kept) >= 4
    d = tmp_path / 'data' / 'words'
    d.mkdir(parents=True)
    files = []
    for i, f in enumerate(kept):
        shutil.copy(f, d / f'{i}.png')
        files.append(str(d / f'{i}.png'))
    batch = _batch(cli, model, files)
    with torch.inference_mode():
        raw, _ = model.tokenizer.read(model(batch))
    labels = [model.charset_adapter(r) for r in raw]
    assert all(labels)
    wrong = {1: None, 3: None}
    for i in wrong:
        labels[i] = wrong[i] = ('b' if labels[i][0] == 'a' else 'a') + labels[i][1:]
    (d / 'gt.txt').write_text(''.join(f'{i}.png {y}\n' for i, y in enumerate(labels)), encoding='utf-8')
    plain = cli.main([ckpt, '--data_root', str(tmp_path / 'data'), 'precision:str=fp32'])
    plain_out = capsys.readouterr().out
    plain_log = open(ckpt + '.log.txt').read()
    assert not os.path.exists(ckpt + '.audit.json')
    results = cli.main([ckpt, '--data_root', str(tmp_path / 'data'), '--audit', '3', '--orders', 'both', 'precision:str=fp32'])
    out = capsys.readouterr().out
    assert results == plain and out.startswith(plain_out) and open(ckpt + '.log.txt').read() == plain_log      # the table is what it was
    assert results[0].num_samples == len(files) and abs(results[0].accuracy - 100 * (len(files) - 2) / len(files)) < 1e-9
    report = json.load(open(ckpt + '.audit.json', encoding='utf-8'))
    assert report['top'] == 3 and report['orders'] == 'both' and report['length_norm'] is False
    ds = report['datasets']['words']
    assert ds['samples'] == len(files) and ds['mismatches'] == 2 and ds['unscorable'] == 0 and len(ds['top']) == 2
    assert sorted(r['index'] for r in ds['top']) == [1, 3] and ds['top'][0]['suspicion'] >= ds['top'][1]['suspicion']
    with torch.inference_mode():
        by_hand = model.score(batch, [[y, r] for y, r in zip(labels, raw)], orders='both').scores.cpu().tolist()
    for r in ds['top']:
        i = r['index']
        assert r['path'] == files[i] and r['label'] == wrong[i] and r['reading'] == raw[i]
        assert abs(r['label_score'] - by_hand[i][0]) <= 2e-3 * (len(labels[i]) + 1) and abs(r['reading_score'] - by_hand[i][1]) <= 2e-3 * (len(raw[i]) + 1)
        assert abs(r['suspicion'] - (r['reading_score'] - r['label_score'])) <= 1e-5
        assert f"{r['path']}  label {r['label']!r}" in out
    assert 'words: 2 of' in out
