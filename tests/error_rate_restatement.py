"""Plain-Python restatement of the error-rate semantics (INTEGRATION.md "Error rates on the device"): a token row becomes a
sequence of units (tokens, code points or words), two sequences are compared by a two-row Levenshtein recurrence.  No torch, no
numpy, nothing shared with the kernels or with conformer_amd.evaluation."""
TOK_CHARS, TOK_DELIM, TOK_SKIP = 0, 1, 2


def tables(vocab, delim_token="|", skip_ids=()):
    """(kinds, cps) of a vocabulary: kind per token, and the code points a token of kind TOK_CHARS spells"""
    kinds = [TOK_SKIP if i in skip_ids else TOK_DELIM if t in (delim_token, " ") else TOK_CHARS for i, t in enumerate(vocab)]
    return kinds, [[ord(c) for c in t] if k == TOK_CHARS else [] for t, k in zip(vocab, kinds)]


def units(ids, count, kinds, cps, kind):
    """The units of the first `count` ids (clamped to the row): "token" -> ids, "char" -> code points, "word" -> tuples of code
    points.  An id outside the vocabulary counts as a skip token."""
    row = [i for i in list(ids)[:max(0, min(int(count), len(ids)))] if 0 <= i < len(kinds) and kinds[i] != TOK_SKIP]
    if kind == "token":
        return [int(i) for i in row]
    words, cur = [], []
    for i in row:
        if kinds[i] == TOK_DELIM:
            if cur:
                words.append(tuple(cur))
            cur = []
        else:
            cur.extend(cps[i])
    if cur:
        words.append(tuple(cur))
    if kind == "word":
        return words
    assert kind == "char", kind
    out = []
    for n, w in enumerate(words):
        if n:
            out.append(0x20)
        out.extend(w)
    return out


def levenshtein(ref, hyp):
    """unit costs; two rows"""
    prev = list(range(len(hyp) + 1))
    for i in range(1, len(ref) + 1):
        cur = [i] + [0] * len(hyp)
        r = ref[i - 1]
        for j in range(1, len(hyp) + 1):
            sub = prev[j - 1] + (0 if r == hyp[j - 1] else 1)
            cur[j] = min(sub, prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return prev[len(hyp)]


def counts(hyp_ids, hyp_count, ref_ids, ref_count, kinds, cps, kind):
    """(errors, hypothesis units, reference units) of one pair"""
    r, h = units(ref_ids, ref_count, kinds, cps, kind), units(hyp_ids, hyp_count, kinds, cps, kind)
    return levenshtein(r, h), len(h), len(r)


def rate(errors, ref_units):
    return errors / ref_units if ref_units else float("nan")
