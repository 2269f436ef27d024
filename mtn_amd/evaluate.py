#!/usr/bin/env python
"""Scoring of generated responses: what stage 4 of run.sh (run.sh:174-196) prints for a result file — Bleu_1..4, ROUGE_L and CIDEr — with
the numbers computed on the device (decode.evaluate_responses; csrc/eval.hip) instead of by coco-caption on the host.

    python evaluate.py RESULT.json REFERENCE.json [--last] [--stopwords FILE] [--per-qa OUT.json]

RESULT.json is what generate.py writes, REFERENCE.json a labelled dialogue file of the same dialogues.  The turns are paired by image_id
and turn index, as utils/get_annotation.py and utils/get_hypotheses.py number them; ``--last`` keeps each dialogue's last turn on both
sides (a result written with --undisclosed-only holds only that one).  A reference turn may carry "answers": [...] (up to 8 texts) next
to or in place of "answer": a multi-reference set.

Text to token ids, host code of this project:
* a sentence is ``text.lower().split()``;
* tokens of coco-caption's punctuation list (PUNCTUATIONS) are dropped;
* ``--stopwords FILE`` applies a stopword file of the reference's format (utils/stopword_filter.py): a line of one column is a pattern to
  delete, of two columns a pattern and its replacement; patterns are regular expressions anchored to the whole word, the first line that
  matches wins, and words that become empty are dropped;
* words map to ids through a dictionary built per evaluation from the words that occur: the model's vocabulary plays no part, so <unk> in a
  hypothesis matches nothing but itself and reference words outside the vocabulary count.
What differs from coco-caption: no PTB tokenisation (contractions are not split), and no METEOR."""
import argparse
import json
import logging
import re

PUNCTUATIONS = ("''", "'", "``", "`", "-LRB-", "-RRB-", "-LCB-", "-RCB-", ".", "?", "!", ",", ":", "-", "--", "...", ";")
_PUNCT = frozenset(p.lower() for p in PUNCTUATIONS)
NAMES = ("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr")
MAX_REF, MAX_LEN = 8, 128


class StopwordFilter:
    """A stopword file of the reference's format: per line `PATTERN` (delete) or `PATTERN REPLACEMENT`; other lines are ignored."""

    def __init__(self, path=None, lines=None):
        if lines is None:
            with open(path, "r") as f:
                lines = f.readlines()
        self.pats = []
        for ln in lines:
            ww = ln.split()
            if len(ww) in (1, 2):
                self.pats.append((re.compile(r"^(?:%s)$" % ww[0]), ww[1] if len(ww) == 2 else ""))

    def __call__(self, words):
        out = []
        for w in words:
            for pat, repl in self.pats:
                if pat.match(w):                                 # the first matching line wins
                    w = pat.sub(repl, w)
                    break
            if w != "":
                out.append(w)
        return out


def tokenize(text, stopwords=None):
    """The words of a sentence: lower-cased, split at white space, without punctuation tokens, through the stopword filter."""
    words = [w for w in text.lower().split() if w not in _PUNCT]
    return stopwords(words) if stopwords is not None else words


def turns(data, last=False):
    """[(key, turn)] of a dialogue file: key = (image_id, turn index), or image_id alone with ``last`` (each dialogue's last turn)."""
    out = []
    for dialog in data["dialogs"]:
        vid, dl = dialog["image_id"], dialog["dialog"]
        if last:
            if dl:
                out.append((vid, dl[-1]))
        else:
            out += [((vid, n), t) for n, t in enumerate(dl)]
    return out


def key_name(key):
    return "%s_%d" % key if isinstance(key, tuple) else "%s (last turn)" % key


def reference_texts(turn, name):
    """The reference texts of a labelled turn: its "answers" list where it has one, else its "answer"."""
    if "answers" in turn:
        texts = turn["answers"]
        if not isinstance(texts, list) or not texts or not all(isinstance(t, str) for t in texts):
            raise SystemExit("evaluate: \"answers\" of reference turn %s is not a non-empty list of strings" % name)
        if len(texts) > MAX_REF:
            raise SystemExit("evaluate: reference turn %s has %d answers (at most %d)" % (name, len(texts), MAX_REF))
        return list(texts)
    if not isinstance(turn.get("answer"), str):
        raise SystemExit("evaluate: reference turn %s has neither \"answer\" nor \"answers\"" % name)
    return [turn["answer"]]


def pair(result, reference, last=False):
    """[(name, hypothesis text, [reference texts])] in the result's order; SystemExit names the first result turn without a reference."""
    refs = dict(turns(reference, last))
    out = []
    for key, turn in turns(result, last):
        name = key_name(key)
        if key not in refs:
            raise SystemExit("evaluate: result turn %s has no reference" % name)
        out.append((name, turn["answer"], reference_texts(refs[key], name)))
    if not out:
        raise SystemExit("evaluate: the result file holds no turn")
    return out


def to_ids(pairs, stopwords=None):
    """(hyps, refs) as token-id lists through a dictionary of the words that occur; SystemExit names an item beyond 128 tokens."""
    ids = {}
    enc = lambda text: [ids.setdefault(w, len(ids)) for w in tokenize(text, stopwords)]
    hyps, refs = [], []
    for name, hyp, texts in pairs:
        h, rs = enc(hyp), [enc(t) for t in texts]
        if len(h) > MAX_LEN or any(len(r) > MAX_LEN for r in rs):
            raise SystemExit("evaluate: %s holds a sentence of more than %d tokens" % (name, MAX_LEN))
        hyps.append(h)
        refs.append(rs)
    return hyps, refs


def score_pairs(pairs, stopwords=None, device=None):
    """The dict of decode.evaluate_responses for [(name, hypothesis text, [reference texts])]."""
    from . import decode
    hyps, refs = to_ids(pairs, stopwords)
    return decode.evaluate_responses(hyps, refs, device=device)


def score_files(result, reference, last=False, stopwords=None, device=None):
    pairs = pair(result, reference, last)
    return pairs, score_pairs(pairs, stopwords, device)


def format_lines(res):
    """The reference's '%s: %.3f' lines (utils/evaluate.py), in the order run.sh:192 reads them; CIDEr is the last."""
    return ["%s: %.3f" % (k, res[k]) for k in NAMES]


def summary(res):
    """The JSON form of a result: the six corpus values and the corpus lengths."""
    out = {k: float(res[k]) for k in NAMES}
    out.update(hyp_len=int(res["hyp_len"]), ref_len=int(res["ref_len"]), n_items=int(len(res["rouge"])))
    return out


def per_qa(pairs, res):
    names = ("guess_1", "guess_2", "guess_3", "guess_4", "match_1", "match_2", "match_3", "match_4", "hyp_len", "closest_ref_len")
    return [dict(dict(zip(names, (int(v) for v in res["stats"][i]))), id=name, ROUGE_L=float(res["rouge"][i]), CIDEr=float(res["cider"][i]))
            for i, (name, _, _) in enumerate(pairs)]


def parse(argv=None):
    p = argparse.ArgumentParser(description="Bleu_1..4, ROUGE_L and CIDEr of a generate.py result file against a labelled dialogue file")
    p.add_argument("result_file", help="result file of generate.py (.json)")
    p.add_argument("reference_file", help="labelled dialogue file (.json)")
    p.add_argument("--last", "-l", action="store_true", help="score only each dialogue's last turn")
    p.add_argument("--stopwords", "-s", default="", type=str, help="stopword file (one column: delete; two columns: replace)")
    p.add_argument("--per-qa", default="", type=str, help="write every turn's statistics, ROUGE_L and CIDEr to this JSON file")
    return p.parse_args(argv)


def main(argv=None):
    args = parse(argv)
    with open(args.result_file, "r") as f:
        result = json.load(f)
    with open(args.reference_file, "r") as f:
        reference = json.load(f)
    sw = StopwordFilter(args.stopwords) if args.stopwords else None
    pairs, res = score_files(result, reference, last=args.last, stopwords=sw)
    for line in format_lines(res):
        print(line)
    if args.per_qa:
        with open(args.per_qa, "w") as f:
            json.dump(dict(summary(res), items=per_qa(pairs, res)), f, indent=4)
    logging.debug("%d turns scored", len(pairs))
    return res


if __name__ == "__main__":
    main()
