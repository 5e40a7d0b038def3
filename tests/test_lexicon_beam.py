"""GPU tests of the lexicon-constrained beam search: the constrained selection kernel alone against the CPU
restatement (tests/lexicon_reference.py), the whole search's decisions against a replay of the restatement from the traced logits, the
exhaustive property against the oracle's teacher-forced log-probabilities, consistency with the unconstrained search, the untouched
`lexicon=None` path, the guards, the refusals and read.py.

The bounds are section 18's (tests/test_beam.py), since the same arithmetic produces the scores: 4e-5 * (step + 1) for a step's scores against
the float64 restatement on the same logits, 8e-3 for a whole search's scores against the CPU oracle."""
import functools
import random

import pytest
import torch

import beam_reference as R
import lexicon_reference as LR
from gpu_util import DEV, native
from oracle.synth import CONFIGS, synth_images, synth_state_dict
from parseq_amd.configs import CHARSET_94_FULL
from parseq_amd.lexicon import Lexicon
from parseq_amd.tokenizer import Tokenizer

pytestmark = pytest.mark.gpu

NEG_INF = float('-inf')
LDT = 32
# the whole-search inputs of tests/test_beam.py: the synthetic head's <eos> bias and the image seeds.  Checked ON THE CPU with the oracle-driven
# restatement under the shared lexicon below (W = 3, max_length = 5, 8 crops): no (image, step) decision of 48 has a gap under twice the score
# bound, the smallest gap is 1.9e-3 (parseq-tiny, seed 101) / 2.7e-2 (parseq, seed 105) — test_whole_search_decisions asserts it again.
EOS_BIAS = 2.25
SEARCH_SEED = {'parseq-tiny': 101, 'parseq': 105}
SEARCH_B, SEARCH_W, SEARCH_MAXLEN = 8, 3, 5
WHOLE_SCORE_BAR = 8e-3
TOK = Tokenizer(CHARSET_94_FULL)


def score_bound(step):
    return 4e-5 * (step + 1)


def _random_words(n, seed, longest):
    """Words over the 94 characters, the first eight of them favoured so that the words share prefixes."""
    rng = random.Random(seed)
    pool = CHARSET_94_FULL[:8] * 6 + CHARSET_94_FULL
    return [''.join(rng.choice(pool) for _ in range(rng.randint(1, longest))) for _ in range(n)]


# -------------------------------------------------------------------------------------------------------------------
# 1. the step kernel alone
# -------------------------------------------------------------------------------------------------------------------
def _run_step(st, B, W, C, eos_id, pad_id, table=None):
    nat, lib = native()
    d = dict(tok=st['tok'].to(DEV, torch.int32).contiguous(), scores=st['scores'].to(DEV, torch.float32).contiguous(),
             finished=st['finished'].to(DEV, torch.uint8).contiguous(), lengths=st['lengths'].to(DEV, torch.int32).contiguous(),
             parent=torch.full((B * W,), -7, dtype=torch.int32, device=DEV), picked=torch.full((B * W,), -7, dtype=torch.int32, device=DEV),
             nodes=st['nodes'].to(DEV, torch.int32).contiguous(), words=st['words'].to(DEV, torch.int32).contiguous())
    lg = st['logits'].to(DEV, torch.float32).contiguous()
    tb = (st['table'] if table is None else table).to(DEV, torch.int32).contiguous()
    with nat.guard(lg):
        nat.check(lib.parseq_op_beam_step_lexicon(nat.ptr(lg), B, W, C, st['step'], nat.ptr(d['tok']), LDT, nat.ptr(d['scores']), nat.ptr(d['finished']),
                                                  nat.ptr(d['lengths']), nat.ptr(d['parent']), nat.ptr(d['picked']), eos_id, pad_id, nat.stream_ptr(lg),
                                                  nat.ptr(tb), tb.shape[0], nat.ptr(d['nodes']), nat.ptr(d['words'])))
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in d.items()}


def _reference_step(st, B, W, eos_id, pad_id):
    table = st['table'].tolist()
    out = []
    for b in range(B):
        rows = slice(b * W, (b + 1) * W)
        out.append(LR.step_image(st['logits'][rows], [float(s) for s in st['scores'][rows]], st['finished'][rows].tolist(), st['lengths'][rows].tolist(),
                                 st['tok'][rows].tolist(), st['nodes'][rows].tolist(), st['words'][rows].tolist(), table, st['step'], eos_id, pad_id))
    return out


def _compare_step(got, want, W, step):
    worst = 0.0
    for b, st in enumerate(want):
        rows = slice(b * W, (b + 1) * W)
        assert got['parent'][rows].tolist() == st.parent
        assert got['picked'][rows].tolist() == st.picked
        assert got['tok'][rows].tolist() == st.hist
        assert got['finished'][rows].tolist() == st.finished
        assert got['lengths'][rows].tolist() == st.lengths
        assert got['nodes'][rows].tolist() == st.nodes
        assert got['words'][rows].tolist() == st.words
        for g, w in zip(got['scores'][rows].tolist(), st.scores):
            if w == NEG_INF:
                assert g == NEG_INF
            else:
                worst = max(worst, abs(g - w))
    assert worst <= score_bound(step), f'score error {worst:.3e} > {score_bound(step):.3e}'
    return worst


@functools.lru_cache(maxsize=None)
def _step_forest(C, B):
    """A tokenizer of C - 1 characters (class ids: <eos> 0, the characters 1 .. C - 1, as the head has them) and one trie per image: 14
    random words of one to six characters and a chain of five characters that no other word shares, whose inner nodes have one child and
    whose last node has <eos> as its only exit."""
    tok = Tokenizer(''.join(chr(0x100 + i) for i in range(C - 1)))
    rng = random.Random(100 * C + B)
    lists = []
    for b in range(B):
        pool = list(range(1, 6)) * 6 + list(range(1, C - 5))
        ids = [[rng.choice(pool) for _ in range(rng.randint(1, 6))] for _ in range(14)]
        ids.append([C - 1 - (k + b) % 5 for k in range(5)])
        lists.append(ids)
    lex, roots = Lexicon.forest([[tok._ids2tok(w) for w in ids] for ids in lists], tok)
    assert lex.next.shape[1] == C and lex.skipped == 0
    return lex, roots.tolist(), lists


def _walk(table, root, ids):
    n = root
    for c in ids:
        n = int(table[n, c])
        assert n >= 0
    return n


KINDS = ('start', 'middle', 'only_eos', 'one_child', 'tie', 'bad_child', 'bad_root')


def _state(kind, B, W, C, seed, eos_id, pad_id, bos_id):
    """Inputs of one constrained step: logits on a 0.25 grid (a permutation per row, |logit| <= 30), distinct per-beam scores, every live
    beam at the node of a prefix of one of its image's words (the histories are random tokens: the kernel copies them, no more)."""
    lex, roots, lists = _step_forest(C, B)
    table = lex.next.clone()
    g = torch.Generator().manual_seed(seed)
    rng = random.Random(seed)
    rows = B * W
    logits = torch.stack([(torch.randperm(C, generator=g).float() - C // 2) * 0.25 for _ in range(rows)])
    assert logits.abs().max() <= 30
    st = dict(step=0, logits=logits, table=table, tok=torch.full((rows, LDT), pad_id, dtype=torch.int64), scores=torch.full((rows,), NEG_INF),
              finished=torch.zeros(rows, dtype=torch.int64), lengths=torch.zeros(rows, dtype=torch.int64),
              nodes=torch.full((rows,), -1, dtype=torch.int64), words=torch.full((rows,), -1, dtype=torch.int64))
    st['tok'][:, 0] = bos_id
    if kind in ('start', 'bad_root'):
        st['scores'][::W] = 0.0
        st['nodes'][::W] = torch.tensor(roots)
        if kind == 'bad_root':      # image 0 past the table, image 1 (if any) negative with a live score, the last image valid when B == 3
            st['nodes'][0] = lex.num_nodes + 3
            if B > 1:
                st['nodes'][W] = -5
        return st
    step = st['step'] = 3
    for r in range(rows):
        b, w = divmod(r, W)
        what = ('live', 'finished', 'dead')[w % 3]
        if w == 0 or (kind == 'tie' and w == 1):
            what = 'live'
        if what == 'dead':
            continue
        st['scores'][r] = -1.0 - 7.0 * torch.rand((), generator=g).item()
        word_k = rng.randrange(14)
        ids = lists[b][word_k]
        if what == 'live':
            prefix = ids[:rng.randrange(len(ids))]
            if w == 0 and kind == 'only_eos':
                prefix = lists[b][14]
            if w == 0 and kind == 'one_child':
                prefix = lists[b][14][:2]
            st['nodes'][r] = _walk(table, roots[b], prefix)
            st['tok'][r, 1:step + 1] = torch.randint(1, C, (step,), generator=g)
            st['lengths'][r] = step
        else:
            n = min(len(ids), step - 1)
            st['nodes'][r] = _walk(table, roots[b], ids)
            st['words'][r] = int(table[st['nodes'][r], eos_id])
            assert st['words'][r] >= 0
            st['tok'][r, 1:n + 1] = torch.randint(1, C, (n,), generator=g)
            st['tok'][r, n + 1] = eos_id
            st['finished'][r], st['lengths'][r] = 1, n
    if kind == 'tie' and W > 1:           # beams 0 and 1 of every image: the same score (the image's best), row and node
        for b in range(B):
            st['scores'][b * W + 1] = st['scores'][b * W] = -0.5
            st['logits'][b * W + 1] = st['logits'][b * W]
            st['nodes'][b * W + 1] = st['nodes'][b * W] = roots[b]
    if kind == 'bad_child':               # every second child id of every live beam's node points past the table
        for r in range(rows):
            n = int(st['nodes'][r])
            if n >= 0 and not st['finished'][r]:
                kids = [c for c in range(1, C) if table[n, c] >= 0]
                for c in kids[::2]:
                    table[n, c] = lex.num_nodes + c
    return st


def _gaps_ok(st, want, B, W, eos_id, kind):
    """Every adjacent-rank gap among the best W + 1 candidates is >= 1e-3 — or, between the two equal beams of 'tie', exactly 0."""
    table = st['table'].tolist()
    for b in range(B):
        rows = slice(b * W, (b + 1) * W)
        top = LR.rank_candidates(st['logits'][rows], [float(s) for s in st['scores'][rows]], st['finished'][rows].tolist(), st['nodes'][rows].tolist(),
                                 table, eos_id)[:W + 1]
        for a, c in zip(top, top[1:]):
            d = a[0] - c[0]
            if not (d >= 1e-3 or (kind == 'tie' and d == 0.0)):
                return False
    return True


@pytest.mark.parametrize('W', [1, 3, 16])
@pytest.mark.parametrize('C', [37, 95, 201])
def test_step_kernel_matches_the_restatement(C, W):
    eos_id, bos_id, pad_id = 0, C, C + 1
    worst, dead_slots, ties = 0.0, 0, 0
    for B in (1, 3):
        for kind in KINDS:
            # inputs are re-drawn (on the CPU, before anything runs) until the gaps are as _gaps_ok wants them
            for attempt in range(200):
                st = _state(kind, B, W, C, 1000 * attempt + 17 * C + W + B, eos_id, pad_id, bos_id)
                want = _reference_step(st, B, W, eos_id, pad_id)
                if _gaps_ok(st, want, B, W, eos_id, kind):
                    break
            else:
                raise AssertionError(('no input with safe gaps', kind, B))
            if kind == 'tie' and W > 1:
                assert all(s.gap == 0.0 for s in want)
                ties += 1
            if kind == 'bad_root':
                assert want[0].parent == [-1] * W and (B == 1 or want[1].parent == [-1] * W) and (B < 3 or want[2].parent[0] == 0)
            if kind == 'only_eos' and W <= 3:      # (among 16 beams the lone <eos> candidate need not rank)
                assert all(eos_id in s.picked for s in want)
            dead_slots += sum(p == -1 for s in want for p in s.parent)
            got = _run_step(st, B, W, C, eos_id, pad_id)
            worst = max(worst, _compare_step(got, want, W, st['step']) / score_bound(st['step']))
            again = _run_step(st, B, W, C, eos_id, pad_id)
            for k in got:
                a, b = (got[k].view(torch.int32), again[k].view(torch.int32)) if got[k].dtype == torch.float32 else (got[k], again[k])
                assert torch.equal(a, b), f'{k}: two runs differ'
    assert dead_slots > 0 and (W == 1 or ties == 2)
    print(f'[lexicon step C={C} W={W}] worst score error {worst:.3f} of the bound, {dead_slots} dead slots')


def test_step_kernel_is_the_unconstrained_one_under_a_trie_that_allows_everything():
    """A one-node table whose every entry is 0 (each character leads back to the root, <eos> spells word 0) removes no candidate: parents,
    tokens, flags, lengths and the bits of the scores are those of parseq_op_beam_step."""
    nat, lib = native()
    C, W, B, eos_id, bos_id, pad_id = 95, 5, 2, 0, 95, 96
    st = _state('middle', B, W, C, 5, eos_id, pad_id, bos_id)
    st['nodes'] = torch.where(st['scores'] > NEG_INF, 0, -1)
    free = torch.zeros(1, C, dtype=torch.int32)
    got = _run_step(st, B, W, C, eos_id, pad_id, table=free)
    d = dict(tok=st['tok'].to(DEV, torch.int32).contiguous(), scores=st['scores'].to(DEV, torch.float32).contiguous(),
             finished=st['finished'].to(DEV, torch.uint8).contiguous(), lengths=st['lengths'].to(DEV, torch.int32).contiguous(),
             parent=torch.full((B * W,), -7, dtype=torch.int32, device=DEV), picked=torch.full((B * W,), -7, dtype=torch.int32, device=DEV))
    lg = st['logits'].to(DEV, torch.float32).contiguous()
    with nat.guard(lg):
        nat.check(lib.parseq_op_beam_step(nat.ptr(lg), B, W, C, st['step'], nat.ptr(d['tok']), LDT, nat.ptr(d['scores']), nat.ptr(d['finished']),
                                          nat.ptr(d['lengths']), nat.ptr(d['parent']), nat.ptr(d['picked']), eos_id, pad_id, nat.stream_ptr(lg)))
    torch.cuda.synchronize()
    for k, v in d.items():
        a, b = (got[k].view(torch.int32), v.cpu().view(torch.int32)) if v.dtype == torch.float32 else (got[k], v.cpu())
        assert torch.equal(a, b), k


# -------------------------------------------------------------------------------------------------------------------
# 2. the whole search, replayed from its traced logits
# -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _weights(name):
    return synth_state_dict(CONFIGS[name], 0, eos_bias=EOS_BIAS)


@functools.lru_cache(maxsize=None)
def _model(name, precision):
    from parseq_amd import create_model
    m = create_model(name, decode_ar=True, refine_iters=0, precision=precision)
    m.model.load_state_dict(_weights(name))
    return m.eval().to(DEV)


@functools.lru_cache(maxsize=None)
def _shared_lexicon():
    return Lexicon(_random_words(40, 7, 7), TOK)       # words of up to 7 characters: the longest cannot finish in 6 steps


@functools.lru_cache(maxsize=None)
def _oracle_search(name):
    cfg = CONFIGS[name]
    images = synth_images(SEARCH_B, cfg, seed=SEARCH_SEED[name])
    return LR.beam_search(R.oracle_step_logits(_weights(name), cfg, images, SEARCH_W), SEARCH_B, SEARCH_W, SEARCH_MAXLEN + 1, cfg.bos_id, cfg.eos_id,
                          cfg.pad_id, _shared_lexicon().next)


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('name', ['parseq-tiny', 'parseq'])
def test_whole_search_decisions(name, precision):
    """The restatement replayed from the traced logits makes the decisions the device made: parents and histories at every step, the final
    tokens, lengths, flags and words, scores within the step bound.  A decision whose float64 gap does not exceed that bound is skipped and
    its image drops out from there on; at most 2 % of the (image, step) decisions may be (here: none of 48)."""
    cfg = CONFIGS[name]
    lex = _shared_lexicon()
    steps, B, W = SEARCH_MAXLEN + 1, SEARCH_B, SEARCH_W
    limits = torch.tensor([score_bound(i) for i in range(steps)], dtype=torch.float64)
    ora = _oracle_search(name)                  # the crops, checked on the CPU with the oracle's logits
    assert int((ora.gaps <= 2 * limits).sum()) <= 0.02 * B * steps
    assert (ora.finished == 1).any() and (ora.words >= 0).any()

    images = synth_images(B, cfg, seed=SEARCH_SEED[name])
    m = _model(name, precision)
    with torch.inference_mode():
        out = m.model.beam_search(m.tokenizer, images.to(DEV), W, SEARCH_MAXLEN, trace=True, lexicon=lex)
    torch.cuda.synchronize()
    res = {k: v.cpu() for k, v in vars(out).items()}
    rep = LR.beam_search(lambda h: res['trace_logits'][h.shape[1] - 1], B, W, steps, cfg.bos_id, cfg.eos_id, cfg.pad_id, lex.next)
    valid = torch.ones(B, dtype=torch.bool)
    skipped, worst = 0, 0.0
    for i in range(steps):
        assert torch.equal(res['trace_tokens_in'][i].long().view(B, W, steps)[valid], rep.tokens_in[i].view(B, W, steps)[valid]), f'histories of step {i}'
        for b in range(B):
            if valid[b] and rep.gaps[b, i] <= limits[i]:
                valid[b] = False
                skipped += 1
        assert torch.equal(res['trace_parent'][i].long().view(B, W)[valid], rep.parents[i][valid]), f'parents of step {i}'
        got, want = res['trace_score'][i].view(B, W)[valid], rep.step_scores[i][valid]
        assert torch.equal(got == NEG_INF, want == NEG_INF)
        d = (got.double() - want).abs()
        d = d[~torch.isnan(d)]
        worst = max(worst, d.max().item() / score_bound(i))
        assert d.max().item() <= score_bound(i), f'step {i}: score error {d.max().item():.3e}'
    print(f'[lexicon decisions {name} {precision}] skipped {skipped} of {B * steps}, worst score error {worst:.3f} of the bound, least gap {rep.gaps.min().item():.2e}')
    assert skipped <= 0.02 * B * steps
    assert torch.equal(res['tokens'].long()[valid], rep.tokens[valid])
    assert torch.equal(res['lengths'].long()[valid], rep.lengths[valid]) and torch.equal(res['finished'].long()[valid], rep.finished[valid])
    assert torch.equal(res['words'].long()[valid], rep.words[valid])
    assert torch.equal(res['scores'][valid], res['trace_score'][-1].view(B, W)[valid])
    # every reading is a prefix of a word of the list, a finished one the word itself
    beams = m.tokenizer.decode_beams(out, lex)
    plain = m.tokenizer.decode_beams(out)
    for alts, raw, fin, wid in zip(beams, plain, res['finished'].tolist(), res['words'].tolist()):
        for r, ((label, _), (chars, _)) in enumerate(zip(alts, raw)):
            assert (label == chars == lex.words[wid[r]]) if fin[r] else (wid[r] == -1 and any(w.startswith(chars) for w in lex.words))


# -------------------------------------------------------------------------------------------------------------------
# 3. exhaustive: per-image lexicons no larger than the beam, against the oracle
# -------------------------------------------------------------------------------------------------------------------
EXH_B, EXH_W, EXH_MAXLEN, EXH_SEED = 8, 4, 5, 301


@functools.lru_cache(maxsize=None)
def _exhaustive_reference(name):
    """Per image four distinct words of one to five characters, and the oracle's teacher-forced log-probability of each."""
    cfg = CONFIGS[name]
    images = synth_images(EXH_B, cfg, seed=EXH_SEED)
    lists = []
    for b in range(EXH_B):
        words = []
        for w in _random_words(12, 50 + b, EXH_MAXLEN):
            if w not in words and len(words) < EXH_W:
                words.append(w)
        assert len(words) == EXH_W
        lists.append(words)
    step_logits = R.oracle_step_logits(_weights(name), cfg, images, EXH_W)
    seqs = [TOK._tok2ids(w) for ws in lists for w in ws]
    scores = torch.tensor(LR.teacher_forced_scores(step_logits, seqs, cfg.bos_id, cfg.eos_id, cfg.pad_id), dtype=torch.float64).view(EXH_B, EXH_W)
    return images, lists, scores


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('name', ['parseq-tiny', 'parseq'])
def test_exhaustive_search_against_the_oracle(name, precision):
    """A trie of at most W words drops no candidate: every image returns exactly its four words, finished, best first, each at the
    oracle's teacher-forced sum of log_softmax within 8e-3 (section 18's bar for whole-search scores), in the oracle's order wherever
    the oracle's gap exceeds that bar; `words` leads back to the strings."""
    images, lists, want = _exhaustive_reference(name)
    lex, roots = Lexicon.forest(lists, TOK)
    m = _model(name, precision)
    with torch.inference_mode():
        res = m.beam_search(images.to(DEV), EXH_W, EXH_MAXLEN, lexicon=lex.to(DEV), roots=roots)
        beams = m.tokenizer.decode_beams(res, lex)
        chars = m.tokenizer.decode_beams(res)
    assert res.finished.cpu().tolist() == [[1] * EXH_W] * EXH_B
    scores, words = res.scores.cpu().double(), res.words.cpu().tolist()
    worst, compared = 0.0, 0
    for b in range(EXH_B):
        assert sorted(words[b]) == list(range(b * EXH_W, (b + 1) * EXH_W))
        assert [lex.words[k] for k in words[b]] == [s for s, _ in beams[b]] == [s for s, _ in chars[b]]
        assert sorted(s for s, _ in beams[b]) == sorted(lists[b])
        assert all(x >= y for x, y in zip(scores[b].tolist(), scores[b].tolist()[1:]))
        order = sorted(range(EXH_W), key=lambda k: -want[b, k].item())
        for r, k in enumerate(words[b]):
            worst = max(worst, abs(scores[b, r].item() - want[b, k - b * EXH_W].item()))
        ranked = [want[b, k].item() for k in order]
        if min(x - y for x, y in zip(ranked, ranked[1:])) > WHOLE_SCORE_BAR:
            assert [k - b * EXH_W for k in words[b]] == order
            compared += 1
    print(f'[lexicon exhaustive {name} {precision}] worst |dscore| {worst:.3e} (bar {WHOLE_SCORE_BAR:.0e}), order compared on {compared} of {EXH_B} images')
    assert worst <= WHOLE_SCORE_BAR and compared >= EXH_B // 2


def test_root_outside_the_table_starts_an_image_dead():
    name = 'parseq-tiny'
    images, lists, _ = _exhaustive_reference(name)
    lex, roots = Lexicon.forest(lists, TOK)
    m = _model(name, 'bf16x3')
    bad = roots.clone()
    bad[2], bad[5] = lex.num_nodes, -1
    with torch.inference_mode():
        want = m.beam_search(images.to(DEV), EXH_W, EXH_MAXLEN, lexicon=lex, roots=roots)
        got = m.beam_search(images.to(DEV), EXH_W, EXH_MAXLEN, lexicon=lex, roots=bad)
    torch.cuda.synchronize()
    ok = torch.tensor([b not in (2, 5) for b in range(EXH_B)])
    for k in ('tokens', 'lengths', 'finished', 'words'):
        assert torch.equal(getattr(got, k).cpu()[ok], getattr(want, k).cpu()[ok]), k
    assert torch.equal(got.scores.cpu()[ok].view(torch.int32), want.scores.cpu()[ok].view(torch.int32))
    cfg = CONFIGS[name]
    assert (got.scores.cpu()[~ok] == NEG_INF).all() and (got.tokens.cpu()[~ok] == cfg.pad_id).all()
    assert (got.words.cpu()[~ok] == -1).all() and (got.finished.cpu()[~ok] == 0).all() and (got.lengths.cpu()[~ok] == 0).all()
    assert m.tokenizer.decode_beams(got, lex)[2] == []


# -------------------------------------------------------------------------------------------------------------------
# 4. beside the unconstrained search
# -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
def test_consistency_with_the_unconstrained_search(precision):
    """Lexicons of the strings an unconstrained W = 4 search of the same crops finished.  Per image (`Lexicon.forest`: at most four words, so
    the constrained search is exhaustive) every one of the image's strings comes back, at the unconstrained score within the whole-search
    bar: the constraint removes candidates and changes no number.  Under ONE lexicon of all the crops' strings that is no theorem — a word
    of another crop, pruned early by the unconstrained search in favour of prefixes of no word, can now hold a slot to the end — so there
    only the scores are compared, wherever a crop's own string is returned."""
    name = 'parseq'
    cfg = CONFIGS[name]
    images = synth_images(8, cfg, seed=SEARCH_SEED[name]).to(DEV)
    m = _model(name, precision)
    with torch.inference_mode():
        free = m.beam_search(images, 4, SEARCH_MAXLEN)
        strings = m.tokenizer.decode_beams(free)
        fin = free.finished.cpu().tolist()
        # (the empty reading, <eos> at once, is no word of a lexicon)
        found = [[(s, lp) for (s, lp), f in zip(alts, fl) if f and s] for alts, fl in zip(strings, fin)]
        vocabulary = sorted({s for alts in found for s, _ in alts})
        assert len(vocabulary) >= 4
        own, roots = Lexicon.forest([[s for s, _ in alts] for alts in found], m.tokenizer)
        shared = Lexicon(vocabulary, m.tokenizer)
        assert own.skipped == 0 and shared.skipped == 0
        con = m.beam_search(images, 4, SEARCH_MAXLEN, lexicon=own, roots=roots)
        got = m.tokenizer.decode_beams(con, own)
        con_shared = m.beam_search(images, 4, SEARCH_MAXLEN, lexicon=shared)
        got_shared = m.tokenizer.decode_beams(con_shared, shared)
    worst, n, n_shared = 0.0, 0, 0
    for alts, mine, cfin, theirs, sfin in zip(found, got, con.finished.cpu().tolist(), got_shared, con_shared.finished.cpu().tolist()):
        assert [f for f in cfin if f] == [1] * len(alts)         # the image's words, all finished, and dead slots
        mine = {s: lp for (s, lp), f in zip(mine, cfin) if f}
        assert sorted(mine) == sorted(s for s, _ in alts)
        theirs = {s: lp for (s, lp), f in zip(theirs, sfin) if f}
        assert all(s in vocabulary for s in theirs)
        for s, lp in alts:
            worst, n = max(worst, abs(mine[s] - lp)), n + 1
            if s in theirs:
                worst, n_shared = max(worst, abs(theirs[s] - lp)), n_shared + 1
    print(f'[lexicon vs unconstrained {precision}] {n} strings of {len(vocabulary)} words ({n_shared} again under the shared lexicon), '
          f'worst |dscore| {worst:.3e} (bar {WHOLE_SCORE_BAR:.0e})')
    assert n >= 8 and n_shared >= 4 and worst <= WHOLE_SCORE_BAR


def test_without_a_lexicon_the_search_is_the_one_it_was():
    from parseq_amd.model import BeamResult
    m = _model('parseq', 'bf16x3')
    x = synth_images(5, CONFIGS['parseq'], seed=11).to(DEV)
    with torch.inference_mode():
        a = m.model.beam_search(m.tokenizer, x, 3, 6)
        con = m.beam_search(x, 3, 6, lexicon=_shared_lexicon())      # a constrained search in between leaves nothing behind
        b = m.beam_search(x, 3, 6, lexicon=None, roots=None)
        c = m.beam_search(x, 3, 6)
    torch.cuda.synchronize()
    assert type(a) is type(b) is type(c) is BeamResult and not hasattr(b, 'words')
    assert isinstance(con, BeamResult) and con.words.shape == (5, 3) and con.words.dtype == torch.int32
    for other in (b, c):
        assert torch.equal(a.tokens, other.tokens) and torch.equal(a.scores.view(torch.int32), other.scores.view(torch.int32))
        assert torch.equal(a.lengths, other.lengths) and torch.equal(a.finished, other.finished)


# -------------------------------------------------------------------------------------------------------------------
# 5. refusals of the library, read.py
# -------------------------------------------------------------------------------------------------------------------
def test_library_refusals():
    nat, lib = native()
    name = 'parseq-tiny'
    cfg = CONFIGS[name]
    m = _model(name, 'bf16x3')
    x = synth_images(4, cfg, seed=3).to(DEV)
    B, W, steps = 4, 2, 4
    plan = m.model._plan(B * W)
    table = _shared_lexicon().table(DEV)

    def call(tb, nodes, words_ok=True, short=0, width=W):
        rows = B * max(width, 1)
        outs = [torch.full((rows * steps,), -7, dtype=torch.int32, device=DEV), torch.full((rows,), -7.0, dtype=torch.float32, device=DEV),
                torch.full((rows,), -7, dtype=torch.int32, device=DEV), torch.full((rows,), 7, dtype=torch.uint8, device=DEV),
                torch.full((rows,), -7, dtype=torch.int32, device=DEV)]
        need = lib.parseq_beam_lexicon_workspace_bytes(plan, B, width, steps)
        ws = torch.empty(max(need, 1 << 20), dtype=torch.uint8, device=DEV)
        status = lib.parseq_forward_beam_lexicon(plan, nat.ptr(x), nat.dtype_code(x.dtype), B, width, steps, nat.ptr(outs[0]), nat.ptr(outs[1]),
                                                 nat.ptr(outs[2]), nat.ptr(outs[3]), None, nat.ptr(ws), (need - short) if short else ws.numel(),
                                                 nat.stream_ptr(x), nat.ptr(tb) if tb is not None else None, nodes, None,
                                                 nat.ptr(outs[4]) if words_ok else None)
        torch.cuda.synchronize()
        untouched = bool((outs[0] == -7).all() and (outs[1] == -7.0).all() and (outs[2] == -7).all() and (outs[3] == 7).all() and (outs[4] == -7).all())
        return status, untouched, need

    plain = lib.parseq_beam_workspace_bytes(plan, B, W, steps)
    status, untouched, need = call(table, table.shape[0])
    assert status == 0 and not untouched and plain < need <= plain + 2 * 256 * ((B * W * 4 + 255) // 256)
    assert call(None, table.shape[0])[:2] == (-1, True) and b'trie' in lib.parseq_last_error()
    assert call(table, 0)[:2] == (-1, True) and b'trie_nodes' in lib.parseq_last_error()
    assert call(table, table.shape[0], words_ok=False)[:2] == (-1, True)
    assert call(table, table.shape[0], short=1)[:2] == (-1, True) and b'workspace' in lib.parseq_last_error()
    assert call(table, table.shape[0], width=17)[:2] == (-1, True) and lib.parseq_beam_lexicon_workspace_bytes(plan, B, 17, steps) == 0
    # the operator hook
    z = torch.zeros(W, 95, device=DEV)
    i32 = torch.zeros(W * LDT, dtype=torch.int32, device=DEV)
    u8 = torch.zeros(W, dtype=torch.uint8, device=DEV)
    for tb, n in ((None, 5), (table, 0)):
        assert lib.parseq_op_beam_step_lexicon(nat.ptr(z), 1, W, 95, 0, nat.ptr(i32), LDT, nat.ptr(z), nat.ptr(u8), nat.ptr(i32), None, nat.ptr(i32), 0, 96,
                                               nat.stream_ptr(z), nat.ptr(tb) if tb is not None else None, n, nat.ptr(i32), nat.ptr(i32)) == -1
    # the Python surface on the device: a table of another head, a deeper decoder
    from parseq_amd import create_model
    with pytest.raises(ValueError, match='lexicon table'):
        m.beam_search(x, 2, lexicon=Lexicon(['12'], Tokenizer('0123456789')))
    deep = create_model(name, dec_depth=2, precision='bf16x3').eval().to(DEV)
    with pytest.raises(ValueError, match='dec_depth'):
        deep.beam_search(x, 2, lexicon=_shared_lexicon())
    assert lib.parseq_beam_lexicon_workspace_bytes(deep.model._plan(8), 4, 2, 4) == 0 and b'dec_depth' in lib.parseq_last_error()


def test_read_cli_lexicon(tmp_path, monkeypatch, capsys):
    Image = pytest.importorskip('PIL.Image')
    import read as read_cli
    from oracle.make_resize_golden import make_input
    files = []
    for i, (h, w) in enumerate([(40, 150), (32, 128)]):
        f = tmp_path / f'crop{i}.png'
        Image.fromarray(make_input(h, w, 1 - i % 2), 'RGB').save(f)
        files.append(str(f))
    words = _random_words(30, 21, 6)
    listing = tmp_path / 'words.txt'
    listing.write_text('\n'.join(words) + '\n')
    m = _model('parseq', 'bf16x3')
    monkeypatch.setattr(read_cli, 'load_from_checkpoint', lambda ckpt, **kw: m)
    read_cli.main(['pretrained=parseq', '--images', *files, '--device', DEV, '--lexicon', str(listing)])
    out = capsys.readouterr().out.splitlines()[1:]
    assert len(out) == 2
    for f, line in zip(files, out):
        assert line.startswith(f + ': ') and line[len(f) + 2:] in words
    read_cli.main(['pretrained=parseq', '--images', *files, '--device', DEV, '--lexicon', str(listing), '--nbest', '3', '--beam', '6'])
    block = capsys.readouterr().out.splitlines()[1:]
    assert len(block) == 8 and [block[0], block[4]] == out
    for k in (0, 4):
        alts = [line.split(None, 1) for line in block[k + 1:k + 4]]
        assert all(line.startswith('    ') for line in block[k + 1:k + 4])
        assert alts[0][1] == block[k].split(': ', 1)[1]
        assert all(float(a[0]) >= float(b[0]) for a, b in zip(alts, alts[1:]))
        assert all(any(w.startswith(a[1]) for w in words) for a in alts)
