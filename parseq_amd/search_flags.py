"""The search flags of the command lines (read.py, test.py, tools/tune_fusion.py): what --beam / --lexicon / --priors / --lm / --pattern /
--lm-weight / --char-bonus / --match / --refine-beams ask for, which of them go together, and the arguments of `beam_search` /
`lexicon_match` / `BeamEvaluator` they turn into.  One set of composition and refusal rules for every command line: a contradiction ends
in `parser.error`.  The resolvers read `args.nbest` and `args.boxes` too; a command line without those flags sets them (test.py: the
N-best is the whole beam, no boxes).  --auto-rotate / --upright-bias have their rules at the end of the module: they
choose the crops every other flag then works on, so they compose with all of them but --polygons.  --candidates / --expect of read.py and
--audit of test.py score given strings instead of searching for one: they refuse every search flag, as does
--analyse of test.py."""
from argparse import SUPPRESS
from collections import namedtuple

LEXICON_BEAM = 8      # --beam under --lexicon when none is given
MATCH_N = 8           # --match without a number
LM_ORDER = 3          # --lm without --lm-order


def load_word_list(path):
    """The words of a lexicon file: one per line, surrounding white space and empty lines dropped."""
    with open(path, encoding='utf-8') as fh:
        return [w for w in (line.strip() for line in fh) if w]


def load_word_counts(path):
    """(words, counts) of a lexicon file with priors: per non-empty line a word and, after white space, its count (a number, not negative)."""
    words, counts = [], []
    with open(path, encoding='utf-8') as fh:
        for number, line in enumerate(fh, 1):
            fields = line.split()
            if not fields:
                continue
            try:
                if len(fields) != 2 or not float(fields[1]) >= 0 or float(fields[1]) == float('inf'):
                    raise ValueError
            except ValueError:
                raise ValueError(f'{path}, line {number}: expected a word and its count, got {line.strip()!r}') from None
            words.append(fields[0])
            counts.append(float(fields[1]))
    return words, counts


def build_automaton(model, kind, args):
    """The automaton of --priors / --lm / --pattern for the model's charset, on the device."""
    from parseq_amd.automaton import Automaton
    if kind == 'priors':
        automaton = Automaton.from_lexicon(*load_word_counts(args.lexicon), model.tokenizer, fold_case=True)
    elif kind == 'lm':
        with open(args.lm, encoding='utf-8') as fh:
            texts = [line.rstrip('\r\n') for line in fh]
            automaton = Automaton.ngram([t for t in texts if t.strip()], args.lm_order or LM_ORDER, model.tokenizer, fold_case=True)      # (blank lines separate, they are no empty sequences)
    else:
        automaton = Automaton.pattern(args.pattern, model.tokenizer)
    return automaton.to(args.device)


def resolve_refine(parser, args, list_flag='--nbest N'):
    """(mode, iterations) of --refine-beams, (None, 1) for none; a contradiction ends in parser.error.  `list_flag`: how the command line that
    asks names the flag that makes `args.nbest` positive."""
    if args.refine_beams is None:
        if args.refine_iters is not None:
            parser.error('--refine-iters needs --refine-beams')
        return None, 1
    if args.lexicon is None and args.nbest <= 0:
        parser.error(f'--refine-beams needs {list_flag} or --lexicon FILE')
    iters = 1 if args.refine_iters is None else args.refine_iters
    if iters < 1:
        parser.error('--refine-iters must be at least 1')
    if args.refine_beams == 'score' and iters != 1:
        parser.error('--refine-beams score runs once: --refine-iters must be 1')
    if args.refine_beams == 'edit' and args.lexicon is not None:
        parser.error('--refine-beams edit is not allowed with --lexicon (an edited reading can leave the list); use score')
    return args.refine_beams, iters


def resolve_match(parser, args):
    """N of --match, None without it; a contradiction ends in parser.error."""
    if args.match is None:
        return None
    if args.lexicon is None:
        parser.error('--match needs --lexicon FILE')
    if args.beam is not None:
        parser.error('--match is not a beam search: not with --beam')
    if args.refine_beams == 'edit':
        parser.error('--match with --refine-beams edit: an edited reading can leave the list (the candidates of --match are rescored already)')
    if not 1 <= args.match <= 16:
        parser.error('--match N must be in [1, 16]')
    if args.nbest > args.match:
        parser.error('--nbest must be at most --match N')
    return args.match


def resolve_automaton(parser, args):
    """(kind, alpha, beta) of the weighted automaton the flags ask for — 'priors', 'lm' or 'pattern', None for none; a contradiction ends in
    parser.error."""
    import math
    kinds = [k for k, on in (('priors', args.priors), ('lm', args.lm is not None), ('pattern', args.pattern is not None)) if on]
    if len(kinds) > 1:
        parser.error('--priors, --lm and --pattern are one automaton each: give one of them')
    if args.priors and args.lexicon is None:
        parser.error('--priors needs --lexicon FILE')
    if args.lm_order is not None and args.lm is None:
        parser.error('--lm-order needs --lm FILE')
    if args.lm_order is not None and not 1 <= args.lm_order <= 4:
        parser.error('--lm-order must be in [1, 4]')
    if not kinds:
        if args.lm_weight is not None or args.char_bonus is not None:
            parser.error('--lm-weight and --char-bonus need --priors, --lm or --pattern')
        return None, 1.0, 0.0
    if args.lexicon is not None and not args.priors:
        parser.error(f'--{kinds[0]} with --lexicon: the search walks one table (--lexicon FILE --priors makes the list the prior)')
    if args.refine_beams is not None or args.match is not None:
        parser.error(f'--{kinds[0]} with --refine-beams or --match: refinement under a weighted automaton is not defined')
    if args.boxes:
        parser.error(f'--{kinds[0]} is a beam search: not with --boxes')
    alpha = 1.0 if args.lm_weight is None else args.lm_weight
    beta = 0.0 if args.char_bonus is None else args.char_bonus
    if not (math.isfinite(alpha) and math.isfinite(beta)):
        parser.error('--lm-weight and --char-bonus must be finite')
    return kinds[0], alpha, beta


def resolve_search(parser, args):
    """(beam width, N) of the search the flags ask for, (None, 0) for none; a contradiction ends in parser.error."""
    if args.lexicon is not None or args.lm is not None or args.pattern is not None:
        nbest = args.nbest if args.nbest > 0 else 1
        beam = args.beam if args.beam is not None else max(LEXICON_BEAM, nbest)
        if beam < nbest:
            parser.error('--beam must be at least --nbest')
        return beam, nbest
    if args.beam is not None and (args.nbest <= 0 or args.beam < args.nbest):
        parser.error('--beam needs --nbest N with N <= the beam width')
    return args.beam, args.nbest


SearchFlags = namedtuple('SearchFlags', 'kind alpha beta match beam nbest refine refine_iters')


def resolve_flags(parser, args, list_flag='--nbest N'):
    """All of the above in the order their refusals take precedence: SearchFlags(kind, alpha, beta, match, beam, nbest, refine, refine_iters)."""
    kind, alpha, beta = resolve_automaton(parser, args)
    match = resolve_match(parser, args)
    beam, nbest = resolve_search(parser, args)
    refine, refine_iters = resolve_refine(parser, args, list_flag)
    return SearchFlags(kind, alpha, beta, match, beam, nbest, refine, refine_iters)


def add_evaluation_flags(parser):
    """The search flags of a command line that evaluates (test.py, tools/tune_fusion.py), named as read.py names them; there is no --nbest
    (the whole beam is evaluated) and no --boxes."""
    parser.add_argument('--beam', type=int, default=None, metavar='W',
                        help=f'Evaluate a beam search of this width and its W-best list (default under --lexicon / --lm / --pattern: {LEXICON_BEAM})')
    parser.add_argument('--lexicon', default=None, metavar='FILE', help='One word list (one word per line) for every dataset: the search is constrained to it')
    parser.add_argument('--priors', action='store_true', help='With --lexicon: a second column holds counts, the words are a prior')
    parser.add_argument('--lm', default=None, metavar='FILE', help='Fuse a character n-gram model counted from this text file into the search')
    parser.add_argument('--lm-order', type=int, default=None, dest='lm_order', metavar='N', help=f'Order of --lm, 1 to 4 (default {LM_ORDER})')
    parser.add_argument('--pattern', default=None, metavar='REGEX', help='Read only what fully matches this regular expression')
    parser.add_argument('--lm-weight', type=float, default=None, dest='lm_weight', metavar='A', help='Weight of the prior of --priors / --lm / --pattern (default 1)')
    parser.add_argument('--char-bonus', type=float, default=None, dest='char_bonus', metavar='B', help='Added per character read, with --priors / --lm / --pattern (default 0)')
    parser.add_argument('--match', type=int, nargs='?', const=MATCH_N, default=None, metavar='N',
                        help=f'With --lexicon: read freely, then let the model choose among the N (default {MATCH_N}) nearest words of the list')
    parser.add_argument('--refine-beams', default=None, choices=['edit', 'score'], dest='refine_beams', help="Refine the alternatives with the model's cloze pass and rank them again")
    parser.add_argument('--refine-iters', type=int, default=None, dest='refine_iters', metavar='K', help='Iterations of --refine-beams edit (default 1)')


def search_requested(args) -> bool:
    """Whether any search flag was given: without one an evaluation stays the greedy one."""
    return (args.beam is not None or args.lexicon is not None or args.priors or args.lm is not None or args.lm_order is not None or args.pattern is not None
            or args.lm_weight is not None or args.char_bonus is not None or args.match is not None or args.refine_beams is not None or args.refine_iters is not None)


def resolve_evaluation_flags(parser, args):
    """SearchFlags of a command line made with `add_evaluation_flags`, None without a search flag: read.py's rules with the N-best = the beam."""
    if not search_requested(args):
        return None
    if args.beam is not None and args.beam < 1:
        parser.error('--beam must be at least 1')
    args.nbest, args.boxes = (args.beam if args.beam is not None and args.match is None else 0), False
    return resolve_flags(parser, args, list_flag='--beam W')


def evaluator_arguments(model, args, flags):
    """The keywords of `BeamEvaluator(model, ...)` for resolved `flags`: the tables (lexicon, automaton) are built once and serve every dataset."""
    if flags.kind is not None:
        return dict(beam_width=flags.beam, automaton=build_automaton(model, flags.kind, args), alpha=flags.alpha, beta=flags.beta)
    kwargs = {}
    if args.lexicon is not None:
        from parseq_amd.lexicon import Lexicon
        kwargs['lexicon'] = Lexicon(load_word_list(args.lexicon), model.tokenizer, fold_case=True, max_label_length=model.model.max_label_length).to(args.device)
    if flags.match is not None:
        return dict(kwargs, match=flags.match)
    if flags.refine is not None:
        kwargs.update(refine=flags.refine, refine_iters=flags.refine_iters)
    return dict(kwargs, beam_width=flags.beam)


def evaluation_width(flags) -> int:
    """Hypotheses per image of the search `flags` ask for: the W of the table's Hit@W."""
    return flags.match if flags.match is not None else flags.beam


# ---- --auto-rotate -----------------------------------------------------------------------------------------------
def add_orientation_flags(parser):
    """--auto-rotate / --upright-bias, for read.py and test.py alike."""
    parser.add_argument('--auto-rotate', default=None, choices=['flip', 'auto', 'all'], dest='auto_rotate', metavar='MODE',
                        help="Read every crop in several quarter turns and keep the one the model reads best: 'flip' tries 0 and 180 degrees, "
                             "'all' 0, 90, 180 and 270, 'auto' 90 and 270 for a crop more than 1.5 times as high as wide and 0 and 180 otherwise")
    parser.add_argument('--upright-bias', type=float, default=None, dest='upright_bias', metavar='X',
                        help="With --auto-rotate: a prior of X nats on every crop's first view (default 0)")


def resolve_orientation(parser, args):
    """(mode, bias) of --auto-rotate, None without it; a contradiction ends in parser.error.  Reads `args.polygons` where the command line has it."""
    import math
    if args.auto_rotate is None:
        if args.upright_bias is not None:
            parser.error('--upright-bias needs --auto-rotate MODE')
        return None
    if getattr(args, 'polygons', None) is not None:
        parser.error('--auto-rotate with --polygons: a polygon has no corner order to shift; cut the regions as quadrilaterals (--regions)')
    bias = 0.0 if args.upright_bias is None else args.upright_bias
    if not math.isfinite(bias):
        parser.error('--upright-bias must be finite')
    return args.auto_rotate, bias


# ---- --lines ------------------------------------------------------------------------------------------------------
LINE_OVERLAP, LINE_SEP = 0.25, 0.25


def add_line_flags(parser):
    """--lines [--line-overlap F] [--line-sep F] of read.py."""
    parser.add_argument('--lines', action='store_true',
                        help='Every image (or region of --regions) is a whole text line: read it as overlapping windows stitched by character position; '
                             'composes with --boxes and --regions only')
    parser.add_argument('--line-overlap', type=float, default=None, dest='line_overlap', metavar='F',
                        help=f'With --lines: the share of a window its neighbour repeats, 0 to 0.75 (default {LINE_OVERLAP})')
    parser.add_argument('--line-sep', type=float, default=None, dest='line_sep', metavar='F',
                        help=f'With --lines: two readings of a character closer than F line heights are one character (default {LINE_SEP}; 0 keeps both)')


def resolve_lines(parser, args):
    """(overlap, sep) of --lines, None without it; a contradiction ends in parser.error.  The greedy reading of a line composes with --boxes
    and --regions; a search, a rotation or --polygons does not reach across windows."""
    import math
    if not args.lines:
        if args.line_overlap is not None or args.line_sep is not None:
            parser.error('--line-overlap and --line-sep need --lines')
        return None
    if search_requested(args) or args.nbest > 0:
        parser.error('--lines reads greedily: not with --nbest, --beam, --lexicon, --match, --priors, --lm, --pattern or --refine-beams')
    if args.auto_rotate is not None or args.upright_bias is not None:
        parser.error('--lines does not turn its windows: not with --auto-rotate')
    if getattr(args, 'polygons', None) is not None:
        parser.error('--lines with --polygons: cut the lines as quadrilaterals (--regions)')
    overlap = LINE_OVERLAP if args.line_overlap is None else args.line_overlap
    sep = LINE_SEP if args.line_sep is None else args.line_sep
    if not 0.0 <= overlap <= 0.75:
        parser.error('--line-overlap must be in [0, 0.75]')
    if not (math.isfinite(sep) and sep >= 0.0):
        parser.error('--line-sep must be finite and at least 0')
    return overlap, sep


# ---- --candidates / --expect / --audit ----------------------------------------------------------------------------
AUDIT_TOP = 20


def parse_orders_flag(text):
    """--orders: 'forward', 'mirrored', 'both', or a number K of orderings drawn as training draws them."""
    if text in ('forward', 'mirrored', 'both'):
        return text
    try:
        k = int(text)
    except ValueError:
        raise ValueError(f"--orders must be forward, mirrored, both or a number, got {text!r}") from None
    if not 1 <= k <= 16:
        raise ValueError('--orders K must be in [1, 16]')
    return k


def _absent_flags(args, **defaults):
    """The flags of this section stay out of the parsed namespace unless they are given (`argparse.SUPPRESS`): a command line without them
    parses to exactly what it parsed to before.  The resolvers fill in what is absent."""
    for name, value in defaults.items():
        if not hasattr(args, name):
            setattr(args, name, value)


def add_score_flags(parser):
    """--candidates FILE / --expect STRING .. [--orders O] [--length-norm] of read.py."""
    parser.add_argument('--candidates', default=SUPPRESS, metavar='FILE',
                        help='Score given readings instead of reading: one line per image (or region), its candidates separated by tabs (at most 16); '
                             'prints them best first with their log-probabilities')
    parser.add_argument('--expect', nargs='+', default=SUPPRESS, metavar='STRING',
                        help='One expected string per image (or region): prints the free reading, then the log-probabilities of the expected string and of the reading')
    add_order_flags(parser)


def add_order_flags(parser):
    parser.add_argument('--orders', default=SUPPRESS, metavar='O',
                        help="With --candidates / --expect / --audit: the decoding orders a string is scored under — forward (default), mirrored, both, or a number K "
                             'of orderings drawn as training draws them; the score is the log of their mixture')
    parser.add_argument('--length-norm', action='store_true', default=SUPPRESS, dest='length_norm', help='With --candidates / --expect / --audit: rank by score / (length + 1)')


def resolve_orders(parser, args, needs):
    """(orders, normalize) of --orders / --length-norm; `needs`: whether a flag that uses them was given, and how the message names it."""
    on, what = needs
    _absent_flags(args, orders=None, length_norm=False)
    if not on:
        if args.orders is not None or args.length_norm:
            parser.error(f'--orders and --length-norm need {what}')
        return None
    try:
        return ('forward' if args.orders is None else parse_orders_flag(args.orders)), bool(args.length_norm)
    except ValueError as e:
        parser.error(str(e))


ScoreFlags = namedtuple('ScoreFlags', 'candidates expect orders normalize')


def resolve_score(parser, args):
    """ScoreFlags of --candidates / --expect, None without them; a contradiction ends in parser.error.  Scoring replaces the reading: it
    composes with --regions (and --polygons) only."""
    _absent_flags(args, candidates=None, expect=None)
    on = args.candidates is not None or args.expect is not None
    picked = resolve_orders(parser, args, (on, '--candidates FILE or --expect STRING'))
    if not on:
        return None
    if args.candidates is not None and args.expect is not None:
        parser.error('--expect is the one-candidate form of --candidates: give one of them')
    if search_requested(args) or args.nbest > 0:
        parser.error('--candidates / --expect score given strings: not with --nbest, --beam, --lexicon, --match, --priors, --lm, --pattern or --refine-beams')
    if args.auto_rotate is not None or args.upright_bias is not None:
        parser.error('--candidates / --expect score the crop as it is: not with --auto-rotate')
    if args.lines or args.line_overlap is not None or args.line_sep is not None:
        parser.error('--candidates / --expect score one crop against one string: not with --lines')
    if args.boxes:
        parser.error('--candidates / --expect do not localise: not with --boxes')
    return ScoreFlags(args.candidates, args.expect, *picked)


def load_candidates(path):
    """The candidate lists of a --candidates file: one line per crop, the strings separated by tabs (an empty line: one empty string)."""
    with open(path, encoding='utf-8') as fh:
        return [line.rstrip('\r\n').split('\t') for line in fh]


def add_audit_flag(parser):
    """--audit [K] [--orders O] [--length-norm] of test.py."""
    parser.add_argument('--audit', type=int, nargs='?', const=AUDIT_TOP, default=SUPPRESS, metavar='K',
                        help=f'After the table: per dataset the K (default {AUDIT_TOP}) samples whose reading the model prefers most over their label, with both '
                             'log-probabilities; everything goes to <checkpoint>.audit.json')
    add_order_flags(parser)


def resolve_audit(parser, args, flags):
    """(K, orders, normalize) of --audit, None without it; `flags`: the resolved search flags.  A contradiction ends in parser.error."""
    _absent_flags(args, audit=None)
    picked = resolve_orders(parser, args, (args.audit is not None, '--audit'))
    if args.audit is None:
        return None
    if args.audit < 1:
        parser.error('--audit K must be at least 1')
    if flags is not None:
        parser.error('--audit scores the greedy reading against the label: not with a search flag')
    if args.auto_rotate is not None or args.upright_bias is not None:
        parser.error('--audit scores the crop as it is: not with --auto-rotate')
    return (args.audit,) + picked


def add_analysis_flag(parser) -> None:
    """--analyse [K] of test.py."""
    parser.add_argument('--analyse', type=int, nargs='?', const=20, default=None, metavar='K',
                        help='After the table: operation totals, accuracy by label length and the K (default 20) most frequent confusions, deletions '
                             'and insertions per dataset; every table goes to <checkpoint>.errors.json')


def resolve_analysis(parser, args, flags):
    """K of --analyse, None without it; `flags`: the resolved search flags.  A contradiction ends in parser.error."""
    if args.analyse is None:
        return None
    if args.analyse < 1:
        parser.error('--analyse K must be at least 1')
    if flags is not None:
        parser.error('--analyse describes the greedy reading: not with a search flag (the analysis of an N-best is out of scope)')
    return args.analyse


def orientation_prior(bias: float, views: int):
    """The prior of `orient` for --upright-bias: `bias` on the first view, None for no bias."""
    return None if bias == 0.0 else [bias] + [0.0] * (views - 1)
