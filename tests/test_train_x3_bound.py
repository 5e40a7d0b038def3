"""CPU side of the bf16x3 training mode (tests/train_x3_reference.py): the derived bounds of the split-bf16 products can fail and need
not — float32 evaluations of the split formula in two summation orders sit inside both bounds for every operator case of
tests/test_train_x3.py, six deliberate errors sit outside them — and one PARSeq-S training step on the CPU oracle with every Linear
product split stays within half of the fp32 device gate of the exact step.  Plus the Python surface that needs no device."""
import re
from pathlib import Path

import pytest
import torch

import train_x3_reference as X
from oracle import train_gemm_ref as G

CASES = X.x3_cases()
ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_float32_inside_and_mutants_outside(case):
    torch.set_num_threads(8)
    t = G.make_inputs(case)
    want = X.expected(case, t)
    for shuffled in (False, True):
        r = X.ratios(X.emulate_f32(case, t, shuffled), want)
        print(f'{case.name}: float32 {"shuffled stages" if shuffled else "kernel order"} worst error / bound (split, full) {r}')
        assert max(max(v) for v in r.values()) <= 1.0
    coherent = (slice(0, None, 8), slice(0, None, 8))      # where two of the every-eighth positive rows meet
    for mutant in X.mutants_of(case):
        tm = X.mutant_inputs(case, t, mutant)
        ref = want if tm is t else X.expected(case, tm)
        mut = X.expected(case, tm, mutant)
        for name in ('C', 'gelu_out'):
            if name not in ref:
                continue
            got = mut[name][0][0]
            for which, (v, b) in zip(('split', 'full'), ref[name]):
                q = (got - v).abs() / b.clamp_min(1e-300)
                r_all, r_coh = float(q.max()), float(q[coherent].max())
                print(f'{case.name}: mutant {mutant} {name} against {which}: worst error / bound {r_all:.3g}, on the coherent rows {r_coh:.3g}')
                assert r_coh > 1.0, f'{mutant} hides inside the {which} bound'


def test_every_mutant_and_every_kernel_form_is_exercised():
    seen = set()
    for c in CASES:
        seen.update(X.mutants_of(c))
    assert seen == set(X.MUTANTS)
    assert {c.kernel for c in CASES} == set(X.KERNELS_X3.values())
    for k in X.KERNELS_X3.values():
        assert {c.plan()[0] > 1 for c in CASES if c.kernel == k} == {False, True}, k
        assert {c.K for c in CASES if c.kernel == k} >= {32, 96, 1472}, k
    assert any(-(-c.M // 128) * -(-c.N // 128) >= 600 and c.K == 64 for c in CASES)


def test_split_is_what_the_bound_assumes():
    """|v - hi - lo| <= 2^-16 |v| and |lo| <= 2^-8 (1 + 2^-8) |v| on Gaussian and on the coherent rows: the two facts bound (2) rests on"""
    x = G._operand(torch.Generator().manual_seed(3), 64, 4096, False)
    hi, lo = X.split(x)
    assert bool(((x.double() - hi.double() - lo.double()).abs() <= 2.0 ** -16 * x.double().abs()).all())
    assert bool((lo.double().abs() <= 2.0 ** -8 * (1 + 2.0 ** -8) * x.double().abs()).all())
    assert torch.equal((x - hi).double(), x.double() - hi.double())      # the subtraction is exact in fp32


@pytest.fixture(scope='module')
def train_golden(golden):
    return golden('parseq_train')


def test_one_training_step_under_the_split_on_the_cpu_oracle(train_golden, monkeypatch):
    """One PARSeq-S step on the parseq_train golden with every LINEAR product of the hand-derived backward (2-D operands; attention stays
    exact) evaluated as al@bh + ah@bl + ah@bh in fp32.  Measured: loss identical as printed, memory max-abs 8.5e-5, worst per-tensor
    max-abs / max|exact| 4.7e-5, worst error / fp32 device gate against the exact step 0.21.  Asserted: per-tensor max-abs / max|exact|
    <= 1e-4 (half of the fp32 device gate's 2e-4) and memory max-abs <= 2e-4."""
    from oracle import decoder_backward as DB, encoder_backward as EB, parseq_oracle as O
    from oracle.synth import CONFIGS, synth_state_dict
    from parseq_amd.tokenizer import Tokenizer
    torch.set_num_threads(8)
    g, meta = train_golden
    cfg = CONFIGS['parseq']
    sd = synth_state_dict(cfg, 0)
    tgt = Tokenizer(X.CHARSET_94).encode(meta['labels'])
    perms = g['perms'].long()

    def step():
        with torch.no_grad():
            memory, saved = EB.forward(sd, cfg, g['images'])
            loss, _, grads, dmem = DB.loss_and_grads(sd, cfg, memory, tgt, perms, O.attn_masks_from_perm)
            grads.update(EB.backward(sd, cfg, saved, dmem))
        return float(loss), memory, grads

    exact_mm = DB.mm

    def split_mm(a, b):
        if a.dim() != 2 or b.dim() != 2:
            return exact_mm(a, b)
        (ah, al), (bh, bl) = X.split(a), X.split(b)
        return al @ bh + ah @ bl + ah @ bh

    exact_loss, exact_mem, exact = step()
    monkeypatch.setattr(DB, 'mm', split_mm)
    monkeypatch.setattr(EB, 'mm', split_mm)
    x3_loss, x3_mem, x3 = step()
    mem_err = float((x3_mem - exact_mem).abs().max())
    worst_rel, worst_gate, worst_l2 = (0.0, ''), (0.0, ''), (0.0, '')
    for k, a in exact.items():
        top = float(a.abs().max())
        if top < 1e-7:
            continue
        err = float((x3[k] - a).abs().max())
        worst_rel = max(worst_rel, (err / top, k))
        worst_gate = max(worst_gate, (err / (2e-4 * top + 1e-7), k))
        worst_l2 = max(worst_l2, (float((x3[k].double() - a.double()).norm() / a.double().norm()), k))
    print(f'split step on the CPU oracle: loss {x3_loss:.7f} against {exact_loss:.7f}; memory max-abs {mem_err:.2e}; worst per-tensor max-abs / max|exact| '
          f'{worst_rel[0]:.2e} ({worst_rel[1]}), L2 rel {worst_l2[0]:.2e} ({worst_l2[1]}), error / fp32 device gate {worst_gate[0]:.2f} ({worst_gate[1]})')
    assert len(exact) == 175
    assert abs(x3_loss - exact_loss) <= 1e-5 * exact_loss
    assert 0 < mem_err <= 2e-4
    assert worst_rel[0] <= 1e-4


# ---- the Python surface --------------------------------------------------------------------------------------------------
def test_set_train_precision_rejects_an_unknown_mode_by_naming_the_three():
    from parseq_amd import train

    class System:
        train_precision = 'fp16'
    with pytest.raises(ValueError) as e:
        train._set_train_precision(System(), None)
    assert all(f"'{m}'" in str(e.value) for m in ('fp32', 'bf16', 'bf16x3')) and 'fp16' in str(e.value)


def test_route_names_of_the_x3_kernels_match_the_header():
    from parseq_amd import _native
    assert len(_native.GEMM_KERNELS) == 13 and tuple(_native.GEMM_KERNELS) == tuple(G.KERNELS)
    header = (ROOT / 'include' / 'parseq_hip.h').read_text()
    enum = dict((n.lower(), int(v)) for n, v in re.findall(r'PARSEQ_GEMM_(X3_[KN]{2})\s*=\s*(\d+)', header))
    assert enum == {v: k for k, v in _native.GEMM_KERNELS_X3.items()} == {v: k for k, v in X.KERNELS_X3.items()}
    assert int(re.search(r'#define PARSEQ_ABI_VERSION (\d+)', header).group(1)) == _native.ABI_VERSION == 15
    assert _native.PARSEQ_BF16X3 == X.X3 == int(re.search(r'PARSEQ_BF16X3 = (\d+)', header).group(1))
