"""Host model of astk_pair_stats (include/astk.h) and the named cases the host and GPU tests share: for a pool of
int32 strings and rows (a, b) of indices into it, [dist, sub, del, ins, m1, m2, m3, m4] per row -- the Levenshtein statistics under the
header's forward rule and the clipped n-gram matches of BLEU.  Plain Python integers: the device result has to EQUAL this one.  The
model shares no code with ast_amd.eval (tests/test_pair_stats_host.py holds the two against each other and against textbook
references)."""
import numpy as np

MAX_LEN = 512
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def edit_stats(a, b):
    """(dist, sub, del, ins) of D[La][Lb]: D[i][0] = i insertions, D[0][j] = j deletions; a cell takes the cheapest of diagonal
    (+ 1 sub when the tokens differ), deletion D[i][j-1] + 1, insertion D[i-1][j] + 1, the earlier one among equals, and carries that
    predecessor's counts."""
    a, b = [int(t) for t in a], [int(t) for t in b]
    prev = [(j, 0, j, 0) for j in range(len(b) + 1)]
    for i in range(1, len(a) + 1):
        row = [(i, 0, 0, i)]
        for j in range(1, len(b) + 1):
            dg, lf, up = prev[j - 1], row[j - 1], prev[j]
            ne = 1 if a[i - 1] != b[j - 1] else 0
            cands = ((dg[0] + ne, dg[1] + ne, dg[2], dg[3]), (lf[0] + 1, lf[1], lf[2] + 1, lf[3]), (up[0] + 1, up[1], up[2], up[3] + 1))
            best = cands[0]
            for c in cands[1:]:
                if c[0] < best[0]:
                    best = c
            row.append(best)
        prev = row
    return prev[len(b)]


def clipped_matches(a, b):
    """(m1, .., m4): m_n = sum over the distinct n-grams of min(count in a, count in b); 0 when a string is shorter than n."""
    a, b = [int(t) for t in a], [int(t) for t in b]
    out = []
    for n in range(1, 5):
        ca, cb = {}, {}
        for s, cnt in ((a, ca), (b, cb)):
            for i in range(len(s) - n + 1):
                g = tuple(s[i:i + n])
                cnt[g] = cnt.get(g, 0) + 1
        out.append(sum(min(c, cb.get(g, 0)) for g, c in ca.items()))
    return tuple(out)


def levenshtein(a, b):
    """The textbook two-row distance, written independently of edit_stats."""
    a, b = list(a), list(b)
    prev = list(range(len(a) + 1))
    for j in range(1, len(b) + 1):
        cur = [j] + [0] * len(a)
        for i in range(1, len(a) + 1):
            cur[i] = min(prev[i] + 1, cur[i - 1] + 1, prev[i - 1] + (a[i - 1] != b[j - 1]))
        prev = cur
    return prev[len(a)]


def row_is_bad(lens, Lmax, a, b):
    S = len(lens)
    return not (0 <= a < S and 0 <= b < S and 0 <= lens[a] <= Lmax and 0 <= lens[b] <= Lmax)


def pair_stats(tokens, lens, pairs):
    """(stats (P, 8) int32, n_bad): a bad row (an index outside the pool, a named length outside [0, Lmax]) is eight -1."""
    tokens, lens, pairs = np.asarray(tokens), [int(n) for n in lens], np.asarray(pairs).reshape(-1, 2)
    Lmax = tokens.shape[1]
    out, memo, n_bad = np.zeros((len(pairs), 8), np.int32), {}, 0
    for r, (a, b) in enumerate(pairs.tolist()):
        if row_is_bad(lens, Lmax, a, b):
            out[r] = -1
            n_bad += 1
            continue
        if (a, b) not in memo:
            sa, sb = tokens[a, :lens[a]].tolist(), tokens[b, :lens[b]].tolist()
            memo[a, b] = edit_stats(sa, sb) + clipped_matches(sa, sb)
        out[r] = memo[a, b]
    return out, n_bad


# ---- what the Python layer computes from the statistics
def mbr_edit(lists):
    """Per list of (tokens, score) the member with the least summed edit distance to the others (as its references); ties go to the
    higher score, then the lower index.  Returns (choices, the integer risks of every list)."""
    choices, risks = [], []
    for lst in lists:
        risk = [sum(edit_stats(h, r)[0] for j, (r, _) in enumerate(lst) if j != i) for i, (h, _) in enumerate(lst)]
        risks.append(risk)
        choices.append(max(range(len(lst)), key=lambda i: (-risk[i], lst[i][1], -i)))
    return choices, risks


def error_rate(list_of_references, hypotheses):
    tot = {"S": 0, "D": 0, "I": 0, "N": 0}
    for refs, hyp in zip(list_of_references, hypotheses):
        ids = {}
        h = [ids.setdefault(w, len(ids)) for w in hyp]
        st = [edit_stats(h, [ids.setdefault(w, len(ids)) for w in r]) for r in refs]
        k = min(range(len(refs)), key=lambda r: (st[r][0], r))
        tot["S"] += st[k][1]
        tot["D"] += st[k][2]
        tot["I"] += st[k][3]
        tot["N"] += len(refs[k])
    tot["rate"] = (tot["S"] + tot["D"] + tot["I"]) / tot["N"] if tot["N"] else 0.0
    return tot


# ---- the named cases: the smallest shapes at which the kernel can go wrong
def _pool(strings, Lmax=None, garbage_seed=None):
    """tokens (S, Lmax) and lens of a list of strings; behind the lengths zeros, or with a seed tokens drawn from the strings' own
    alphabet (so a kernel that read them would find matches)."""
    Lmax = Lmax or max(1, max(len(s) for s in strings))
    if garbage_seed is None:
        tokens = np.zeros((len(strings), Lmax), np.int32)
    else:
        alphabet = sorted({int(t) for s in strings for t in s}) or [0]
        tokens = np.random.default_rng(garbage_seed).choice(alphabet, size=(len(strings), Lmax)).astype(np.int32)
    for i, s in enumerate(strings):
        tokens[i, :len(s)] = s
    return tokens, np.asarray([len(s) for s in strings], np.int32)


def _rand(seed, length, symbols):
    return np.random.default_rng(seed).integers(0, symbols, size=length).astype(np.int64).tolist()


def _all_pairs(S):
    return [(a, b) for a in range(S) for b in range(S)]


def _case(strings, pairs, **kw):
    tokens, lens = _pool(strings, **kw)
    return dict(tokens=tokens, lens=lens, pairs=np.asarray(pairs, np.int32).reshape(-1, 2))


def _boundaries(seed, symbols):
    """63, 64 and 65 against 1, 64, 65 and 130, both ways: the last lane of a block, a full block, one column more, three blocks."""
    strings = [_rand(seed + k, n, symbols) for k, n in enumerate((63, 64, 65, 1, 64, 65, 130))]
    pairs = [(a, b) for a in range(3) for b in range(3, 7)]
    return _case(strings, pairs + [(b, a) for a, b in pairs])


def _cap():
    s = [_rand(31, 512, 3), _rand(32, 512, 3), _rand(33, 511, 3), _rand(34, 512, 1000), _rand(35, 512, 1000)]
    s[4][100:400] = s[3][103:403]                            # a long shifted common run: deletions, insertions and high-order matches
    return _case(s, [(0, 1), (2, 1), (1, 2), (3, 4), (3, 3)])


def _bad_rows():
    strings = [_rand(71 + k, n, 4) for k, n in enumerate((5, 9, 0, 12, 7, 3))]
    tokens, lens = _pool(strings, Lmax=12, garbage_seed=7)
    lens = lens.copy()
    lens[4], lens[5] = -1, 13                                # two strings whose length lies outside [0, Lmax]
    S = len(strings)
    pairs = [(0, 1), (-1, 0), (1, 3), (0, S), (S, -1), (4, 0), (0, 4), (2, 3), (5, 1), (1, 5), (3, 3), (I32_MIN, 0), (0, I32_MAX), (3, 1)]
    return dict(tokens=tokens, lens=lens, pairs=np.asarray(pairs, np.int32))


def _p5000():
    rng = np.random.default_rng(81)
    strings = [_rand(82 + k, int(n), 4) for k, n in enumerate(rng.integers(0, 25, size=48))]
    return _case(strings, rng.integers(0, 48, size=(5000, 2)).tolist(), Lmax=24)


def _nbest():
    """32 near-duplicates of one 40-token string, all pairs i < j: what mbr_select_lists launches."""
    rng = np.random.default_rng(91)
    base = rng.integers(4, 60, size=40).tolist()
    strings = []
    for _ in range(32):
        s = list(base)
        for _ in range(int(rng.integers(0, 8))):
            k = int(rng.integers(0, len(s)))
            op = int(rng.integers(0, 3))
            if op == 0:
                s[k] = int(rng.integers(4, 60))
            elif op == 1:
                del s[k]
            else:
                s.insert(k, int(rng.integers(4, 60)))
        strings.append(s)
    return _case(strings, [(i, j) for i in range(32) for j in range(i + 1, 32)])


_EXTREME = (0, -1, I32_MAX, I32_MIN)

CASES = {
    "empty": lambda: _case([[], [7], _rand(11, 512, 5), []], [(0, 0), (0, 3), (0, 1), (1, 0), (0, 2), (2, 0)]),
    "identical": lambda: _case([_rand(12, 40, 9), _rand(12, 40, 9), _rand(13, 130, 2), _rand(13, 130, 2)], [(0, 1), (0, 0), (2, 3), (3, 3)]),
    "single": lambda: _case([[5], [5], [6]], [(0, 1), (0, 2), (2, 0)]),
    "boundaries": lambda: _boundaries(20, 6),
    "boundaries-2-symbols": lambda: _boundaries(40, 2),
    "boundaries-3-symbols": lambda: _boundaries(50, 3),
    "cap": _cap,
    "clipping": lambda: _case([[3, 3, 3, 3], [3, 3], [1, 2, 1, 2, 1, 2, 1], [1, 2, 1, 2], [2, 1, 2]], _all_pairs(5)),
    "short": lambda: _case([[1], [2], [1, 2], [2, 1], [1, 1], [1, 2, 3], [1, 2, 1], [3, 2, 1], [1, 2, 3, 4], [1, 2, 3, 4, 5]], _all_pairs(10)),
    "extreme-ids": lambda: _case([[_EXTREME[t] for t in _rand(60 + k, 1 + 3 * k, 4)] for k in range(8)] + [[I32_MIN], [I32_MAX], [-1], [0]],
                                 _all_pairs(12)),
    "repeated": lambda: _case([_rand(14, 70, 3), _rand(15, 66, 3)], [(0, 1), (1, 0), (0, 1), (0, 1), (1, 0), (1, 1), (0, 1)]),
    "one-pair": lambda: _case([_rand(16, 21, 4), _rand(17, 19, 4)], [(1, 0)]),
    "p5000": _p5000,
    "garbage": lambda: _case([_rand(18 + k, n, 3) for k, n in enumerate((17, 0, 5, 16, 1, 9))], _all_pairs(6), Lmax=40, garbage_seed=3),
    "bad-rows": _bad_rows,
    "n-best": _nbest,
}
ALL_CASES = list(CASES)

_RESULT = {}


def case(name):
    return CASES[name]()


def result(name):
    """(case dict, (stats, n_bad) of the model), computed once and shared; callers leave both unchanged."""
    if name not in _RESULT:
        c = case(name)
        _RESULT[name] = (c, pair_stats(c["tokens"], c["lens"], c["pairs"]))
    return _RESULT[name]
