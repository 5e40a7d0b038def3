"""DESIGN.md section 29 restated in plain numpy float64: the window plan of a text line and the stitch of its windows' characters.
Nothing here imports parseq_amd; the tests compare the package's plan and the library's kernel against these functions exactly."""
import math

import numpy as np

MAX_WINDOWS = 64


def line_windows(h, w, img_size, overlap=0.25, aspect=1.0):
    """[(x0, ww)] of a line of h x w pixels."""
    img_h, img_w = img_size
    if h < 1 or w < 1 or not 0.0 <= overlap <= 0.75 or not 0.25 <= aspect <= 4.0:
        raise ValueError('bad plan parameters')
    ww = max(1, math.floor(h * img_w / img_h * aspect + 0.5))
    if w <= ww:
        return [(0, w)]
    ov = math.floor(ww * overlap + 0.5)
    s = max(1, ww - ov)
    K = math.ceil((w - ww) / s) + 1
    if K > MAX_WINDOWS:
        raise ValueError(f'{K} windows')
    return [(min(k * s, w - ww), ww) for k in range(K)]


def stitch_line(tokens, lengths, probs, centres, boxes, win, C, img_size, min_sep, max_out):
    """One line.  tokens int [K, L], lengths int [K], probs fp32 [K, L], centres fp32 [K, L, 2], boxes fp32 [K, L, 4], win int [K, 3]
    = (x0, ww, h) per window, min_sep a float64 in source pixels.
    Returns dict(len, tokens [max_out], probs, boxes [max_out, 4], x, src [max_out, 2], confidence)."""
    f64, f32 = np.float64, np.float32
    img_h, img_w = img_size
    K, L = tokens.shape
    min_sep = f64(min_sep)
    delta = min_sep / f64(2)
    with np.errstate(all='ignore'):
        sx = [f64(int(win[k][1])) / f64(img_w) for k in range(K)]
        sy = [f64(int(win[k][2])) / f64(img_h) for k in range(K)]
        ox = [f64(int(win[k][0])) for k in range(K)]
        X = np.asarray(ox, f64).reshape(K, 1) + np.asarray(centres, f32)[:, :, 0].astype(f64).reshape(K, L) * np.asarray(sx, f64).reshape(K, 1)
        cuts = [(f64(int(win[k + 1][0])) + f64(int(win[k][0]) + int(win[k][1]))) / f64(2) for k in range(K - 1)]
        n = [min(max(int(lengths[k]), 0), L) for k in range(K)]
        # 1, 2: candidates and ownership
        kept = []
        for k in range(K):
            lo = -np.inf if k == 0 else cuts[k - 1] - delta
            hi = np.inf if k == K - 1 else cuts[k] + delta
            kept.append([i for i in range(n[k]) if 0 <= int(tokens[k, i]) < C and bool(lo <= X[k, i]) and bool(X[k, i] < hi)])
        # 3: every seam on its own, on the lists of step 2
        dropped = set()
        if min_sep > 0:
            for k in range(K - 1):
                matched = set()
                for b in kept[k + 1]:
                    best, bd = None, None
                    for a in kept[k]:
                        if a in matched or int(tokens[k, a]) != int(tokens[k + 1, b]):
                            continue
                        d = np.abs(X[k, a] - X[k + 1, b])
                        if bool(d < min_sep) and (best is None or bool(d < bd)):
                            best, bd = a, d
                    if best is not None:
                        matched.add(best)
                        if not bool(probs[k + 1, b] > probs[k, best]):
                            dropped.add((k + 1, b))
                        else:
                            dropped.add((k, best))
        # 4: (window, position) order
        surv = [(k, i) for k in range(K) for i in kept[k] if (k, i) not in dropped]
        # 5: fp64 products in a fixed order
        conf = f64(1.0)
        for k in range(K):
            q = f64(1.0)
            for kk, i in surv:
                if kk == k:
                    q = q * f64(probs[k, i])
            conf = conf * q
        p_eos = f64(probs[K - 1, n[K - 1]]) if K > 0 and n[K - 1] < L else f64(1.0)
        conf = f32(conf * p_eos)
        # 6
        out = dict(len=len(surv), tokens=np.full(max_out, -1, np.int32), probs=np.zeros(max_out, f32), boxes=np.zeros((max_out, 4), f32),
                   x=np.zeros(max_out, f64), src=np.full((max_out, 2), -1, np.int32), confidence=conf)
        for r, (k, i) in enumerate(surv[:max_out]):
            out['tokens'][r] = tokens[k, i]
            out['probs'][r] = probs[k, i]
            out['x'][r] = X[k, i]
            out['src'][r] = (k, i)
            bx = boxes[k, i]
            out['boxes'][r] = (f32(ox[k] + f64(bx[0]) * sx[k]), f32(f64(0.0) + f64(bx[1]) * sy[k]), f32(ox[k] + f64(bx[2]) * sx[k]), f32(f64(0.0) + f64(bx[3]) * sy[k]))
    return out


def stitch_lines(tokens, lengths, probs, centres, boxes, win, line_first, C, img_size, min_sep, max_out):
    """All lines of a call: rows line_first[l] .. line_first[l + 1] - 1 are line l.  Returns dict of stacked arrays (len int32 [lines], ...)."""
    per = []
    for l in range(len(line_first) - 1):
        a, b = int(line_first[l]), int(line_first[l + 1])
        per.append(stitch_line(tokens[a:b], lengths[a:b], probs[a:b], centres[a:b], boxes[a:b], win[a:b], C, img_size, min_sep[l], max_out))
    return dict(len=np.array([p['len'] for p in per], np.int32), tokens=np.stack([p['tokens'] for p in per]), probs=np.stack([p['probs'] for p in per]),
                boxes=np.stack([p['boxes'] for p in per]), x=np.stack([p['x'] for p in per]), src=np.stack([p['src'] for p in per]),
                confidence=np.array([p['confidence'] for p in per], np.float32))
