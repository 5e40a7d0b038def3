"""Host tests of character localisation: the NumPy geometry on hand-made maps, the CPU restatement of the map
(tests/attn_map_reference.py) against the goldens minted from the reference (tools/make_golden_attn.py), and the refusals of the Python
surface that need no device."""
import numpy as np
import pytest
import torch

import attn_map_reference as AR
from oracle.synth import CONFIGS, synth_images, synth_state_dict

GRIDS, block_map, load_attn_golden = AR.GRIDS, AR.block_map, AR.load_attn_golden


@pytest.mark.parametrize('gh,gw,ph,pw', GRIDS)
def test_one_hot_map_gives_exactly_its_cell(gh, gw, ph, pw):
    for t in (0, gw - 1, 3 * gw + 5, gh * gw - 1):
        a = np.zeros((1, 1, gh * gw)); a[0, 0, t] = 1.0
        centres, boxes, peak, mass = AR.geometry(a, [0], gh, gw, ph, pw)
        r, c = divmod(t, gw)
        np.testing.assert_allclose(centres[0, 0], [(c + 0.5) * pw, (r + 0.5) * ph], rtol=0, atol=1e-12)
        np.testing.assert_allclose(boxes[0, 0], [c * pw, r * ph, (c + 1) * pw, (r + 1) * ph], rtol=0, atol=1e-12)
        assert peak[0, 0] == t and mass[0, 0] == 1.0


@pytest.mark.parametrize('gh,gw,ph,pw', GRIDS)
@pytest.mark.parametrize('k', [1, 2, 5])
@pytest.mark.parametrize('m', [1, 2, 5])
def test_uniform_block_gives_exactly_its_rectangle(gh, gw, ph, pw, k, m):
    r0, c0 = 2, 3
    centres, boxes, peak, mass = AR.geometry(block_map(gh, gw, r0, c0, k, m), [0], gh, gw, ph, pw)
    np.testing.assert_allclose(boxes[0, 0], [c0 * pw, r0 * ph, (c0 + m) * pw, (r0 + k) * ph], rtol=0, atol=1e-10)
    np.testing.assert_allclose(centres[0, 0], [(c0 + m / 2) * pw, (r0 + k / 2) * ph], rtol=0, atol=1e-10)
    assert peak[0, 0] == r0 * gw + c0 and mass[0, 0] == pytest.approx(1.0 / (k * m))      # every cell ties: the lowest index


@pytest.mark.parametrize('gh,gw,ph,pw', GRIDS)
def test_box_touching_a_border_is_clipped(gh, gw, ph, pw):
    # two cells in the first column and one far to the right: the box's left edge would lie left of the image
    a = np.zeros((gh, gw)); a[0, 0] = 0.45; a[1, 0] = 0.45; a[0, gw - 1] = 0.10
    centres, boxes, _, _ = AR.geometry(a.reshape(1, 1, -1), [0], gh, gw, ph, pw)
    cx = 0.9 * 0.5 * pw + 0.1 * (gw - 0.5) * pw
    var = 0.9 * (0.5 * pw - cx) ** 2 + 0.1 * ((gw - 0.5) * pw - cx) ** 2 + pw * pw / 12
    assert cx - np.sqrt(3 * var) < 0                       # the case is what it claims to be
    assert boxes[0, 0, 0] == 0.0 and boxes[0, 0, 1] == 0.0
    assert boxes[0, 0, 2] == pytest.approx(min(cx + np.sqrt(3 * var), gw * pw), abs=1e-10)
    assert centres[0, 0, 0] == pytest.approx(cx, abs=1e-10)
    # a block in the last rows / columns ends on the border, not past it
    _, boxes, _, _ = AR.geometry(block_map(gh, gw, gh - 2, gw - 2, 2, 2), [0], gh, gw, ph, pw)
    np.testing.assert_allclose(boxes[0, 0], [(gw - 2) * pw, (gh - 2) * ph, gw * pw, gh * ph], rtol=0, atol=1e-10)
    assert boxes[0, 0, 2] <= gw * pw and boxes[0, 0, 3] <= gh * ph


def test_peak_ties_resolve_to_the_lowest_index():
    gh, gw, ph, pw = GRIDS[0]
    a = np.full((1, 1, gh * gw), 0.5 / (gh * gw - 2)); a[0, 0, 70] = 0.25; a[0, 0, 17] = 0.25
    _, _, peak, mass = AR.geometry(a, [0], gh, gw, ph, pw)
    assert peak[0, 0] == 17 and mass[0, 0] == 0.25


def test_invalid_rows_give_zeros_and_minus_one():
    gh, gw, ph, pw = GRIDS[0]
    rng = np.random.default_rng(0)
    a = rng.random((2, 5, gh * gw)); a /= a.sum(-1, keepdims=True)
    centres, boxes, peak, mass = AR.geometry(a, [1, 4], gh, gw, ph, pw)
    assert (centres[0, 2:] == 0).all() and (boxes[0, 2:] == 0).all() and (peak[0, 2:] == -1).all() and (mass[0, 2:] == 0).all()
    assert (peak[0, :2] >= 0).all() and (peak[1] >= 0).all() and (boxes[1, :, 2] > boxes[1, :, 0]).all()


@pytest.fixture(scope='module', params=['parseq-tiny', 'parseq-patch16-224'])
def golden_case(request):
    """(name, cfg, golden arrays, the restatement's map for the golden's tgt_in) — computed once per model."""
    name = request.param
    g, meta = load_attn_golden(name)
    cfg = CONFIGS[name]
    sd = synth_state_dict(cfg, meta['seed'], eos_bias=meta['eos_bias'])
    images = synth_images(meta['candidates'], cfg, seed=meta['crop_seed'])[torch.tensor(meta['candidate_ids'])]
    with torch.inference_mode():
        got = AR.attention_map(sd, cfg, torch.from_numpy(g['tgt_in']), AR.encode(sd, cfg, images))
    return name, cfg, g, got.numpy()


def test_restatement_reproduces_the_reference_maps(golden_case):
    """The reference's own `ca_weights` of the refinement pass.  Measured on the CPU that minted the fixtures: max |difference| 0.0 for both
    models (the restatement issues the reference's operations in the reference's order).  The bound leaves room for another CPU's
    matrix-product summation order only: 1e-6 is about 25 fp32 ulps of a probability near 1 and far below the 4e-2 the largest entries
    reach, so a wrong mask, scale or head mean cannot hide under it."""
    name, cfg, g, got = golden_case
    assert got.shape == g['maps'].shape == (g['tgt_in'].shape[0], cfg.max_label_length + 1, cfg.num_patches)
    d = np.abs(got - g['maps']).max()
    print(f'[{name}] restatement vs reference map: max |d| {d:.3e}, largest entry {g["maps"].max():.3e}')
    assert d <= 1e-6


def test_golden_rows_sum_to_one_and_are_zero_past_the_reading(golden_case):
    name, cfg, g, _ = golden_case
    L = g['maps'].shape[1]
    is_eos = g['tgt_in'] == cfg.eos_id                           # tgt_in is the content: <bos>, then the reading
    lengths = np.where(is_eos.any(-1), is_eos.argmax(-1), L) - 1
    valid = np.arange(L)[None, :] <= lengths[:, None]
    sums = g['maps'].sum(-1)
    assert 1 <= lengths.min() and lengths.max() < L - 1          # the strings end inside the label range: both kinds of row exist
    assert np.abs(sums[valid] - 1.0).max() <= 1e-5              # an fp32 sum of <= 256 terms
    assert (g['maps'][~valid] == 0).all()


def test_label_longer_than_the_model_reads_is_refused():
    from parseq_amd import create_model
    m = create_model('parseq-tiny', precision='fp32')
    with pytest.raises(ValueError, match='max_label_length'):
        m.localize(torch.zeros(1, 3, 32, 128), ['x' * (m.model.max_label_length + 1)])


def test_read_boxes_does_not_compose_with_nbest_or_lexicon(capsys):
    import read
    for extra in (['--nbest', '3'], ['--lexicon', 'words.txt']):
        with pytest.raises(SystemExit) as e:
            read.main(['pretrained=parseq', '--images', 'a.png', '--boxes'] + extra)
        assert e.value.code == 2
        assert '--boxes' in capsys.readouterr().err


def test_scale_box_stretches_each_axis_on_its_own():
    import read
    assert read.scale_box((8.0, 4.0, 64.0, 32.0), (32, 128), (64, 512)) == (32.0, 8.0, 256.0, 64.0)
