#!/usr/bin/env python
"""Response generation with the reference's generate.py flags (generate.py:91-115), so that the `python generate.py ...` line of
run.sh:156-168 (stage 3) decodes a test set on this implementation and writes the result JSON that stage 4 scores.

The reference decodes one QA at a time, each at its own padded shape.  Here a search over D dialogues side by side costs about
as much as a search over one, but decode sessions and their captured graphs are cached per padded shape (decode._session).  So
the QAs are planned first:

* every QA gets a bucket key: its frame counts rounded up to FRAME_STEP, its history / question / caption lengths rounded up to
  TEXT_STEP (DESIGN.md §10 gives the grid and the bucket count it yields on the AVSD test lengths); a first turn's history (the
  lone, masked <blank>) keeps its length of one;
* each bucket is cut into groups of D QAs; the last group is padded with copies of its last QA (their results are dropped), so
  every search of a bucket has one shape and reuses one session and one captured search graph;
* buckets are decoded one after another (the session cache never thrashes), each group's Batch is assembled on the device by
  make_batch into the same tensors (``out=``), and the results go back to qa_id order before output.

Padding does not change a search: padded keys are masked to -1e9 and padded frames are zeroed and masked, as in the reference's
own batches — except in a row whose keys are ALL masked, hence the exception above (tests/test_generate_gpu.py compares every QA with its own unpadded single-QA search).

``--decode-style score`` rides in the same buckets but generates nothing: every QA's candidate responses (``--candidates FILE``; its
own answer without an entry) are scored by decode.score_candidates — one encoder-side pass per QA, the candidates as rows of a
teacher-forced pass, csrc/score.hip — logged best first, written into the result JSON as "scores", and summed up as corpus
perplexity and, where the file names the ground truth, MRR / R@k / mean rank (score_metrics).
"""
import argparse
import copy
import json
import logging
import pickle
import time
from collections import OrderedDict

FRAME_STEP = 64          # bucket grid: frame counts of every feature type rounded up to a multiple of this
TEXT_STEP = 32           # ... history, question and caption lengths to a multiple of this
MAX_SAMPLES = 16         # --samples: the samples of a QA ride in one search (decode.MegaDecodeSession.MAX_W rows)
MBR_MAX_HYP, MBR_MAX_LEN = 16, 128       # --mbr: hypotheses per QA and tokens per hypothesis (include/mtn_hip.h mtn_mbr_select)
CONTRASTIVE_MAX_K = 12   # --contrastive-k: with the three ids the CLI bans and <eos>, the candidates fit a row head of 16 entries
LAUNCH_PASS_D = 8        # dialogues per search where the persistent decode step does not apply (launch-per-sublayer pass)

# the reference train.py's defaults (train.py:57-96) for fields a conf may lack (confs written by older versions)
REFERENCE_TRAIN_DEFAULTS = dict(fea_type=None, include_caption="none", separate_caption=False, cut_a=0, merge_source=0,
                                exclude_video=False, fixed_word_emb=0, nb_blocks=6, d_model=512, d_ff=2048, att_h=8, dropout=0.1,
                                separate_his_embed=0, separate_cap_embed=0, diff_encoder=0, diff_embed=0, diff_gen=0,
                                auto_encoder_ft=None, max_length=20, max_history_length=-1)


def parse(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--gpu", "-g", default=0, type=int, help="GPU ID (negative value indicates CPU)")
    p.add_argument("--test-path", default="", type=str, help="Path to test feature files")
    p.add_argument("--test-set", default="", type=str, help="Filename of test data")
    p.add_argument("--model-conf", default="", type=str, help="Attention model to be output")
    p.add_argument("--model", "-m", default="", type=str, help="Attention model to be output")
    p.add_argument("--maxlen", default=30, type=int, help="Max-length of output sequence")
    p.add_argument("--beam", default=3, type=int, help="Beam width")
    p.add_argument("--penalty", default=2.0, type=float, help="Insertion penalty")
    p.add_argument("--nbest", default=5, type=int, help="Number of n-best hypotheses")
    p.add_argument("--output", "-o", default="", type=str, help="Output generated responses in a json file")
    p.add_argument("--verbose", "-v", default=0, type=int, help="verbose level")
    p.add_argument("--decode-style", default="greedy", type=str, help="greedy, beam_search, sample, contrastive or score")
    p.add_argument("--undisclosed-only", default=0, type=int, help="")
    # (nargs="?": run.sh passes `--labeled-test ${labeled_test}` with labeled_test='' by default, i.e. the bare flag)
    p.add_argument("--labeled-test", default=None, nargs="?", type=str, help="directory to labelled data")
    # this implementation
    p.add_argument("--compute-dtype", default="bf16", choices=["bf16", "fp32"])
    p.add_argument("--dialogues-per-search", default=0, type=int,
                   help="QAs decoded side by side in one search; 0 = the most the persistent decode step takes (16 rows: 16 // beam "
                        "for beam search, 16 for greedy, 16 // samples for sample), %d where it does not apply" % LAUNCH_PASS_D)
    # --decode-style sample: stochastic decoding on the device (temperature / top-k / nucleus), --samples draws per QA, best first
    p.add_argument("--temperature", default=1.0, type=float, help="sample: softmax temperature (0 = arg-max)")
    p.add_argument("--top-k", default=0, type=int, help="sample: keep the k most probable tokens (ties kept; 0 = off)")
    p.add_argument("--top-p", default=1.0, type=float, help="sample: nucleus, the smallest set of tokens with this mass (1 = off)")
    p.add_argument("--samples", default=1, type=int, help="sample: responses drawn per QA (at most %d); the best-scoring one is the answer" % MAX_SAMPLES)
    p.add_argument("--sample-seed", default=1, type=int, help="sample: seed of the random streams (a QA's stream depends on the seed and its qa_id only)")
    # --decode-style contrastive: contrastive search (Su et al. 2022) — among the K most probable tokens the one whose decoder state is
    # least similar to the prefix' states (csrc/contrastive.hip); deterministic, one answer per QA
    p.add_argument("--contrastive-k", default=5, type=int, help="contrastive: candidates per position (1..%d; 1 = greedy)" % CONTRASTIVE_MAX_K)
    p.add_argument("--contrastive-alpha", default=0.6, type=float,
                   help="contrastive: weight of the degeneration penalty against the model's probability (0..1; 0 = greedy)")
    # --decode-style score: nothing is generated — given responses are scored (teacher-forced log-likelihood) and ranked
    p.add_argument("--candidates", default=None, type=str,
                   help='score: JSON {"<image_id>_<turn>": {"candidates": ["text", ...], "gt_index": k}} (gt_index optional); a QA '
                        "without an entry, and every QA without this flag, is scored on its own answer")
    # constrained decoding (beam_search, greedy, sample): the rows of log-probabilities are rewritten on the device before selection
    p.add_argument("--no-repeat-ngram", default=0, type=int, help="no response repeats an n-gram of this size (1..8; 0 = off)")
    p.add_argument("--repetition-penalty", default=1.0, type=float,
                   help="multiply the log-probability of every token a response already holds by this (>= 1; 1 = off)")
    p.add_argument("--min-length", default=1, type=int, help="beam_search / sample: no response ends before this many tokens")
    # diverse beam search (beam_search only): the beam as --beam-groups groups that are penalised for repeating each other's newest token
    p.add_argument("--beam-groups", default=1, type=int, help="beam_search: split the beam into this many groups (divides --beam; 1 = plain beam search)")
    p.add_argument("--diversity-penalty", default=0.0, type=float,
                   help="beam_search: what a group's log-probability of a token loses per hypothesis of an earlier group that just took it (>= 0; needs --beam-groups > 1)")
    # ensemble decoding: further checkpoints combined with --model on the device, per generated token (decode.Ensemble)
    p.add_argument("--ensemble-model", default=[], nargs="+", type=str, help="further checkpoints (PREFIX.pth.tar each), decoded together with --model")
    p.add_argument("--ensemble-conf", default=[], nargs="+", type=str,
                   help="their confs, one per --ensemble-model entry; without this flag every member uses --model-conf")
    p.add_argument("--ensemble-weights", default=None, nargs="+", type=float,
                   help="one weight >= 0 per member, --model's first (normalised to sum 1; default: uniform)")
    p.add_argument("--ensemble-mode", default="prob", choices=["prob", "logprob"],
                   help="prob: log of the weighted mean probability; logprob: weighted mean log-probability, renormalised")
    # minimum-Bayes-risk selection (sample, beam_search): the answer is the hypothesis that agrees most, in n-grams, with the others (csrc/mbr.hip)
    p.add_argument("--mbr", default=0, type=int,
                   help="sample / beam_search: answer with the hypothesis of the largest expected n-gram utility, n-grams up to this order (1..4; 0 = off)")
    p.add_argument("--mbr-weights", default=None, choices=["uniform", "score"],
                   help="mbr: weight of a hypothesis in the expectation: uniform (default), or score = softmax of the hypotheses' scores")
    p.add_argument("--mbr-temperature", default=None, type=float, help="mbr: temperature of the score weights (> 0; default 1)")
    # scoring of the generated answers on the device (mtn_amd.evaluate; csrc/eval.hip): run.sh's stage 4 inside stage 3
    p.add_argument("--evaluate", action="store_true",
                   help="score the answers written to the result JSON: Bleu_1..4, ROUGE_L, CIDEr against the test set's own answers, or with "
                        "--undisclosed-only 1 against the last answers of --labeled-test FILE")
    p.add_argument("--stopwords", default="", type=str, help="evaluate: stopword file applied to hypotheses and references (utils/stopword_filter.py's format)")
    p.add_argument("--no-buckets", action="store_true",
                   help="one QA per search at its own padded shape, as the reference decodes (baseline / debugging)")
    args = p.parse_args(argv)
    args.undisclosed_only = bool(args.undisclosed_only)
    if args.decode_style not in ("greedy", "beam_search", "sample", "contrastive", "score"):
        p.error("--decode-style must be greedy, beam_search, sample, contrastive or score")
    if not 1 <= args.contrastive_k <= CONTRASTIVE_MAX_K:
        p.error("--contrastive-k must be in [1, %d]" % CONTRASTIVE_MAX_K)
    if not 0.0 <= args.contrastive_alpha <= 1.0:
        p.error("--contrastive-alpha must be in [0, 1]")
    if args.decode_style == "contrastive":
        # the search reads ONE decoder's states and takes no row constraint: what it does not combine with ends the run by name
        for on, flag in ((bool(args.ensemble_model), "--ensemble-model"), (args.mbr != 0, "--mbr"), (args.beam_groups > 1, "--beam-groups"),
                         (args.no_repeat_ngram != 0, "--no-repeat-ngram"), (args.repetition_penalty != 1.0, "--repetition-penalty"),
                         (args.candidates is not None, "--candidates")):
            if on:
                p.error("%s does not go with --decode-style contrastive" % flag)
    if args.candidates is not None and args.decode_style != "score":
        p.error("--candidates goes with --decode-style score")
    if not 1 <= args.samples <= MAX_SAMPLES:
        p.error("--samples must be in [1, %d] (the rows of one persistent decode step)" % MAX_SAMPLES)
    if args.temperature < 0 or args.top_k < 0 or not 0 < args.top_p <= 1:
        p.error("--temperature >= 0, --top-k >= 0, 0 < --top-p <= 1")
    if not 0 <= args.no_repeat_ngram <= 8:
        p.error("--no-repeat-ngram must be in [0, 8]")
    if not args.repetition_penalty >= 1.0:
        p.error("--repetition-penalty must be >= 1")
    if args.decode_style == "score" and (args.no_repeat_ngram != 0 or args.repetition_penalty != 1.0):
        p.error("--no-repeat-ngram / --repetition-penalty constrain a search: they do not go with --decode-style score")
    if args.min_length < 0:
        p.error("--min-length must be >= 0")
    if args.beam_groups < 1:
        p.error("--beam-groups must be >= 1")
    if not (args.diversity_penalty >= 0 and args.diversity_penalty < float("inf")):
        p.error("--diversity-penalty must be finite and >= 0")
    if args.decode_style != "beam_search":
        if args.beam_groups > 1:
            p.error("--beam-groups goes with --decode-style beam_search")
        if args.diversity_penalty > 0:
            p.error("--diversity-penalty goes with --decode-style beam_search")
    elif args.beam % args.beam_groups:
        p.error("--beam-groups must divide --beam (%d groups for a beam of %d)" % (args.beam_groups, args.beam))
    elif args.diversity_penalty > 0 and args.beam_groups == 1:
        p.error("--diversity-penalty needs --beam-groups > 1 (one group is the plain beam search)")
    if not 0 <= args.mbr <= 4:
        p.error("--mbr must be in [0, 4]")
    if args.mbr_temperature is not None and not args.mbr_temperature > 0:
        p.error("--mbr-temperature must be > 0")
    if args.mbr == 0 and (args.mbr_weights is not None or args.mbr_temperature is not None):
        p.error("--mbr-weights / --mbr-temperature go with --mbr > 0")
    if args.mbr > 0:
        if args.decode_style not in ("sample", "beam_search"):
            p.error("--mbr selects among several hypotheses: it goes with --decode-style sample or beam_search")
        if args.decode_style == "beam_search" and args.nbest > MBR_MAX_HYP:
            p.error("--mbr takes at most %d hypotheses: --nbest must be <= %d" % (MBR_MAX_HYP, MBR_MAX_HYP))
        if args.maxlen > MBR_MAX_LEN:
            p.error("--mbr takes hypotheses of at most %d tokens: --maxlen must be <= %d" % (MBR_MAX_LEN, MBR_MAX_LEN))
    if args.stopwords and not args.evaluate:
        p.error("--stopwords goes with --evaluate")
    if args.evaluate:
        if args.decode_style == "score":
            p.error("--evaluate scores generated answers: --decode-style score generates nothing")
        if args.undisclosed_only and not args.labeled_test:
            p.error("--evaluate with --undisclosed-only 1 needs --labeled-test FILE: the test set's own last answers are undisclosed")
    args.mbr_weights = args.mbr_weights or "uniform"
    args.mbr_temperature = 1.0 if args.mbr_temperature is None else args.mbr_temperature
    n_members = 1 + len(args.ensemble_model)
    if args.ensemble_conf and len(args.ensemble_conf) != len(args.ensemble_model):
        p.error("--ensemble-conf takes one conf per --ensemble-model entry (%d given for %d)" % (len(args.ensemble_conf), len(args.ensemble_model)))
    if n_members > 8:
        p.error("an ensemble has at most 8 members (--model and 7 --ensemble-model entries)")
    if args.ensemble_weights is not None:
        w = args.ensemble_weights
        if len(w) != n_members:
            p.error("--ensemble-weights takes one weight per member, --model's first (%d given for %d)" % (len(w), n_members))
        if any(not (v >= 0 and v < float("inf")) for v in w) or not sum(w) > 0:
            p.error("--ensemble-weights are finite numbers >= 0, not all of them 0")
    return args


# ---------------------------------------------------------------------------------------------------------------- model
def load_conf(path):
    """<model>.conf = pickled (vocab, argparse.Namespace), as the reference's or this project's train.py writes it.  Fields an
    older conf lacks take the reference train.py's defaults."""
    with open(path, "rb") as f:
        vocab, train_args = pickle.load(f)
    for k, v in REFERENCE_TRAIN_DEFAULTS.items():
        if not hasattr(train_args, k):
            setattr(train_args, k, v)
    return vocab, train_args


def load_state_dict(path):
    """A state_dict in the reference's key schema.  The reference's own train.py pickles the whole nn.Module (train.py:183): that
    needs the reference's classes to unpickle and is refused with a recipe to extract its state_dict."""
    import torch
    how = ("%s holds a pickled nn.Module (what the reference's train.py saves), not a state_dict.  Extract its state_dict where the "
           "reference's mtn.py is importable:\n    python -c \"import torch; m = torch.load('%s', weights_only=False); "
           "torch.save(m.state_dict(), '%s')\"\nand pass that file's prefix to --model." % (path, path, path))
    try:
        sd = torch.load(path, map_location="cpu", weights_only=True)
    except Exception as e:        # weights_only refuses any pickled class that is not a tensor container
        raise SystemExit(how + "\n(torch.load: %s)" % str(e).splitlines()[0]) from None
    if isinstance(sd, torch.nn.Module) or not isinstance(sd, dict) or not all(isinstance(v, torch.Tensor) for v in sd.values()):
        raise SystemExit(how)
    return sd


def build_model(vocab, train_args, ft_sizes, state_dict, compute_dtype, device):
    from . import make_model
    a = train_args
    model = make_model(len(vocab), len(vocab), N=a.nb_blocks, d_model=a.d_model, d_ff=a.d_ff, h=a.att_h, dropout=a.dropout,
                       separate_his_embed=bool(a.separate_his_embed), separate_cap_embed=bool(a.separate_cap_embed),
                       ft_sizes=ft_sizes, diff_encoder=bool(a.diff_encoder), diff_embed=bool(a.diff_embed), diff_gen=bool(a.diff_gen),
                       auto_encoder_ft=a.auto_encoder_ft, compute_dtype=compute_dtype)
    res = model.load_state_dict(state_dict, strict=False)
    params = {n for n, _ in model.named_parameters()}
    missing = [k for k in res.missing_keys if k in params]
    if missing:
        raise SystemExit("checkpoint does not fit the conf's model: %d parameter(s) missing, e.g. %s" % (len(missing), missing[:4]))
    model.to(device).eval()
    model.prepare()
    return model


ENSEMBLE_DATA_FIELDS = ("fea_type", "include_caption", "separate_caption", "max_history_length", "merge_source")


def check_ensemble_confs(confs, names=None):
    """The members of an ensemble read ONE test set and write into ONE vocabulary: every conf (load_conf's pair) must carry the first one's
    token-to-id map and its data-shaping fields (ENSEMBLE_DATA_FIELDS).  SystemExit naming the first member and field that differ."""
    names = names or ["member %d" % i for i in range(len(confs))]
    vocab0, args0 = confs[0]
    for (vocab, a), name in zip(confs[1:], names[1:]):
        if dict(vocab) != dict(vocab0):
            raise SystemExit("ensemble: the vocabulary of %s differs from that of %s (%d and %d tokens): members share one token-to-id map"
                             % (name, names[0], len(vocab), len(vocab0)))
        for f in ENSEMBLE_DATA_FIELDS:
            if getattr(a, f) != getattr(args0, f):
                raise SystemExit("ensemble: %s of %s is %r, of %s %r: members read the same test data"
                                 % (f, name, getattr(a, f), names[0], getattr(args0, f)))


def load_ensemble_confs(model_conf, ensemble_models, ensemble_confs):
    """[(vocab, train_args)] of --model and every --ensemble-model entry (its --ensemble-conf, or --model-conf without that flag), checked."""
    paths = [model_conf] + (list(ensemble_confs) if ensemble_confs else [model_conf] * len(ensemble_models))
    if len(paths) != 1 + len(ensemble_models):
        raise SystemExit("ensemble: one conf per --ensemble-model entry")
    confs = [load_conf(p) for p in paths]
    check_ensemble_confs(confs, ["%s (member %d)" % (p, i) for i, p in enumerate(paths)])
    return confs


# ---------------------------------------------------------------------------------------------------------------- planning
def qa_lengths(data):
    """Per qa_id: (frame counts per feature type, history, question, answer, caption) lengths of data_handler.load's items."""
    out = []
    for it in sorted(data["dialogs"], key=lambda d: d[1]):
        vid = it[0]
        x = tuple(len(f[vid]) if not isinstance(f[vid], tuple) else f[vid][1] for f in (data["features"] or []))
        out.append((x, len(it[2]), len(it[3]), len(it[4]), len(it[6]) if len(it) > 6 else 0))
    return out


def _up(n, step):
    return -(-int(n) // step) * step


def bucket_key(lens, frame_step=FRAME_STEP, text_step=TEXT_STEP):
    """(frames per feature type, history, question, caption), each rounded up to its grid step.  A history of one token is the
    lone <blank> placeholder of a first turn (data_handler.load): every key of it is masked, and attention over a fully masked
    row averages ALL its keys (the reference's softmax over -1e9 everywhere), so its length is kept exactly."""
    x, h, q, _, c = lens
    return tuple(_up(v, frame_step) for v in x), (h if h <= 1 else _up(h, text_step)), _up(q, text_step), _up(c, text_step)


def plan_searches(lens, per_search, buckets=True, frame_step=FRAME_STEP, text_step=TEXT_STEP):
    """Group the QAs (``lens`` = qa_lengths, indexed by qa_id) into searches.  ``per_search``: D, or a function of a bucket's
    padded lengths -> D.  Returns [(qa_ids, n_real, (x_len, h, q, a, c))]: the first n_real ids are distinct QAs, the rest
    copies of the last of them; every search of a bucket has the bucket's D and padded lengths.  ``buckets=False``: one QA per
    search at its own lengths."""
    if not buckets:
        return [([i], 1, (list(l[0]), l[1], l[2], l[3], l[4])) for i, l in enumerate(lens)]
    groups = OrderedDict()
    for i, l in enumerate(lens):
        groups.setdefault(bucket_key(l, frame_step, text_step), []).append(i)
    out = []
    for key in sorted(groups):
        ids = groups[key]
        x, h, q, c = key
        shape = (list(x), h, q, max(lens[i][3] for i in ids), c)      # (answers: not read by a decode; the longest of the bucket)
        D = max(1, int(per_search(shape) if callable(per_search) else per_search))
        for s in range(0, len(ids), D):
            chunk = ids[s:s + D]
            out.append((chunk + [chunk[-1]] * (D - len(chunk)), len(chunk), shape))
    return out


def auto_dialogues(model, device, shape, maxlen, width):
    """The most QAs side by side that the persistent decode step takes at this shape (D x width <= 16 rows, fewer at wide
    feed-forwards), LAUNCH_PASS_D where it does not apply (fp32 models, unsupported widths).  An ensemble (decode.Ensemble) takes the
    smallest count any of its members allows: the step applies to all of them or to none."""
    import types
    import torch
    from .decode import MegaDecodeSession
    x, h, q, _, c = shape
    for D in range(MegaDecodeSession.MAX_W // width, 0, -1):
        e = lambda n: torch.empty(D, max(1, n), device=device)
        probe = types.SimpleNamespace(query=e(q), his=e(h), cap=e(c), fts=[torch.empty(D, max(1, v), 1, device=device) for v in x])
        if MegaDecodeSession.supported(model, probe, maxlen, width):
            return D
    return LAUNCH_PASS_D


# ---------------------------------------------------------------------------------------------------------------- output
def detokenize(tokens, vocablist, eos):
    """generate.py:59-64: words up to (not including) the first <eos>."""
    words = []
    for w in tokens:
        if w == eos:
            break
        words.append(vocablist[w])
    return " ".join(words)


def greedy_text(ys, vocablist, eos):
    """generate.py:71-77: greedy output without its leading <sos>, up to <eos>."""
    return detokenize(list(ys)[1:], vocablist, eos)


def build_result(original, undisclosed_only, answers, scores=None, mbr=None, contrastive=None):
    """{'dialogs': [{'image_id', 'dialog'}]} in file order (generate.py:27-38): every turn, or the last one with undisclosed-only;
    ``answers[qa_id]`` replaces the answer of the qa_id-th output turn; ``scores[qa_id]`` (--decode-style score) becomes its "scores",
    ``mbr[qa_id]`` (--mbr) its "mbr", ``contrastive[qa_id]`` (--decode-style contrastive) its "contrastive"."""
    dialogs, qa = [], 0
    for dialog in original["dialogs"]:
        out = copy.deepcopy(dialog["dialog"][-1:] if undisclosed_only else dialog["dialog"])
        for turn in out:
            turn["answer"] = answers[qa]
            if scores is not None:
                turn["scores"] = scores[qa]
            if mbr is not None:
                turn["mbr"] = mbr[qa]
            if contrastive is not None:
                turn["contrastive"] = contrastive[qa]
            qa += 1
        dialogs.append({"image_id": dialog["image_id"], "dialog": out})
    return {"dialogs": dialogs}


# ---------------------------------------------------------------------------------------------------------------- scoring
def tokenize_answer(text, vocab):
    """An answer's token ids as data_handler.words2ids gives them, without its <sos> / <eos>: unknown words -> <unk>."""
    from .data_handler import words2ids
    return [int(t) for t in words2ids(text, vocab)[1:-1]]


def qa_keys(original, undisclosed_only):
    """Per qa_id (the order of data_handler.load): ("<image_id>_<turn>", the turn's dict) — the key is what the per-QA log line prints."""
    out = []
    for dialog in original["dialogs"]:
        turns = dialog["dialog"][-1:] if undisclosed_only else dialog["dialog"]
        out += [("%s_%d" % (dialog["image_id"], t), qa) for t, qa in enumerate(turns)]
    return out


def load_candidates(spec, original, vocab, undisclosed_only=False, ref_data=None):
    """What --decode-style score scores, per qa_id: dict(key, texts, tokens, gt_index, ranked).  ``spec``: the --candidates JSON (a dict,
    a path to one, or None).  A QA with an entry gets its candidates and its gt_index (None without one; not an index into the
    candidates: ValueError); every other QA is scored on its own answer (ref_data's with undisclosed-only and a labelled test set),
    which is then its ground truth but takes no part in the ranking metrics (``ranked`` False)."""
    if isinstance(spec, str):
        with open(spec, "r") as f:
            spec = json.load(f)
    spec = spec or {}
    out, per_dialog = [], []                                # per_dialog[qa_id]: the index of its dialogue
    for idx, dialog in enumerate(original["dialogs"]):
        per_dialog += [idx] * (1 if undisclosed_only else len(dialog["dialog"]))
    keys = qa_keys(original, undisclosed_only)
    unknown = set(spec) - {k for k, _ in keys}
    if unknown:
        raise ValueError("candidates: no QA is called %s" % sorted(unknown)[:4])
    for qa_id, (key, turn) in enumerate(keys):
        entry = spec.get(key)
        if entry is None:
            own = turn["answer"]
            if undisclosed_only and ref_data is not None:
                rd = ref_data["dialogs"][per_dialog[qa_id]]
                assert rd["image_id"] == original["dialogs"][per_dialog[qa_id]]["image_id"]
                own = rd["dialog"][-1]["answer"]
            texts, gt, ranked = [own], 0, False
        else:
            texts = entry.get("candidates") if isinstance(entry, dict) else None
            if not isinstance(texts, list) or not texts or not all(isinstance(t, str) for t in texts):
                raise ValueError("candidates: %s needs a non-empty list of strings under \"candidates\"" % key)
            gt = entry.get("gt_index")
            if gt is not None and (isinstance(gt, bool) or not isinstance(gt, int) or not 0 <= gt < len(texts)):
                raise ValueError("candidates: gt_index of %s is not an index into its %d candidates" % (key, len(texts)))
            ranked = gt is not None
        out.append(dict(key=key, texts=list(texts), tokens=[tokenize_answer(t, vocab) for t in texts], gt_index=gt, ranked=ranked))
    return out


def score_metrics(qas):
    """The corpus numbers of a scoring run.  ``qas``: per QA dict(score=[...], logp=[...], n_tokens=[...], gt_index=k or None,
    ranked=bool), candidates in input order.  perplexity = exp(-sum logp / sum n_tokens) over the ground-truth answers (every QA with a
    gt_index); over the ``ranked`` QAs, with rank = 1 + the candidates that score higher than the ground truth + the EARLIER ones that
    score the same (ties keep input order): mrr, r@1 / r@5 / r@10 (share of ranks <= k) and mean_rank.  None where nothing counts."""
    import math
    lp = sum(q["logp"][q["gt_index"]] for q in qas if q["gt_index"] is not None)
    nt = sum(q["n_tokens"][q["gt_index"]] for q in qas if q["gt_index"] is not None)
    ranks = []
    for q in qas:
        if q.get("ranked") and q["gt_index"] is not None:
            g, s = q["gt_index"], q["score"]
            ranks.append(1 + sum(1 for j, v in enumerate(s) if v > s[g] or (v == s[g] and j < g)))
    n = len(ranks)
    share = lambda k: sum(1 for r in ranks if r <= k) / n if n else None
    return dict(perplexity=math.exp(-lp / nt) if nt else None, n_answers=sum(1 for q in qas if q["gt_index"] is not None), n_tokens=nt,
                n_ranked=n, ranks=ranks, mrr=sum(1.0 / r for r in ranks) / n if n else None, r1=share(1), r5=share(5), r10=share(10),
                mean_rank=sum(ranks) / n if n else None)


def candidate_order(scores):
    """Candidate indices, best score first; equal scores keep input order."""
    return sorted(range(len(scores)), key=lambda j: (-scores[j], j))


# ---------------------------------------------------------------------------------------------------------------- decoding
def decode_searches(model, corpus, searches, vids, vocab, decode_style, maxlen, beam, penalty, nbest, sampling=None, scoring=None,
                    no_repeat_ngram=0, repetition_penalty=1.0, min_len=1, beam_groups=1, diversity_penalty=0.0, mbr=0, mbr_weights="uniform",
                    mbr_temperature=1.0, contrastive=None):
    """Run the planned searches; returns per qa_id the (n-best list, best score) of beam search, the greedy token list, the
    (tokens, score, log-probabilities, penalties, ranks) of contrastive search (``contrastive``: k / alpha), the
    samples' (tokens, score) pairs, best first (``sampling``: samples / temperature / top_k / top_p / seed), or the candidates'
    score dicts in input order (``scoring``: tokens = per qa_id its candidates' token lists, max_len, width — one session shape
    per bucket).  ``no_repeat_ngram`` / ``repetition_penalty`` constrain beam search, greedy and sample (decode.py; off by default);
    ``min_len``: the shortest response beam search and sample may finish.  ``beam_groups`` / ``diversity_penalty``: diverse beam search
    (beam search only; decode.beam_search_decode_many).  ``mbr`` = N > 0 (beam search and sample): every QA's hypotheses — the n-best list cut
    to ``nbest``, or the samples — come back as (tokens, score, expected utility) triples in minimum-Bayes-risk order of n-gram order N
    (decode.mbr_rerank; uniform weights over samples ride inside the search, decode.sample_decode_many's ``mbr``)."""
    from . import decode
    from .data_handler import make_batch
    from .decode import beam_search_decode_many, greedy_decode_many
    sos, eos, unk, pad = vocab["<sos>"], vocab["<eos>"], vocab["<unk>"], vocab["<blank>"]
    results = {}
    batch, batch_shape = None, None
    con = dict(no_repeat_ngram=int(no_repeat_ngram), repetition_penalty=float(repetition_penalty))
    for ids, n_real, shape in searches:
        x, h, q, a, c = shape
        index = ([vids[i] for i in ids], ids, x, h, q, a, c, len(ids))
        key = (tuple(x), h, q, a, c, len(ids))
        batch = make_batch(corpus, index, pad, separate_caption=True, out=batch if key == batch_shape else None)
        batch_shape = key
        if decode_style == "beam_search":
            res = beam_search_decode_many(model, batch, maxlen, sos, unk, eos, pad, beam=beam, penalty=penalty, nbest=nbest, min_len=min_len,
                                          beam_groups=int(beam_groups), diversity_penalty=float(diversity_penalty), **con)
            if mbr:                  # plain, diverse and ensemble searches hand back the same list: one launch re-ranks the whole search's
                ranked = decode.mbr_rerank([r[0][:nbest] for r in res], mbr, weights=mbr_weights, temperature=mbr_temperature)
                res = [(t, r[1]) for t, r in zip(ranked, res)]
        elif decode_style == "sample":
            # keys = qa_ids: a QA's random stream is the same in any bucket, at any D, with --no-buckets
            in_search = dict(mbr=int(mbr)) if mbr and mbr_weights == "uniform" else {}
            res = decode.sample_decode_many(model, batch, maxlen, sos, eos, pad, keys=ids, banned=(unk, pad, sos), min_len=min_len, penalty=penalty,
                                            **sampling, **con, **in_search)
            if mbr and not in_search:
                res = decode.mbr_rerank(res, mbr, weights=mbr_weights, temperature=mbr_temperature)
        elif decode_style == "contrastive":
            # the ids `sample` bans; the row constraints and ensembles do not apply to this search (generate_response refuses them)
            res = decode.contrastive_decode_many(model, batch, maxlen, sos, eos, pad, k=contrastive["k"], alpha=contrastive["alpha"],
                                                 banned=(unk, pad, sos), min_len=min_len, penalty=penalty)
        elif decode_style == "score":
            # (a padding copy of the last QA rides with one candidate: its rows are dropped)
            cands = [scoring["tokens"][i] if k < n_real else scoring["tokens"][i][:1] for k, i in enumerate(ids)]
            res = decode.score_candidates(model, batch, cands, sos, eos, pad, penalty=penalty, max_len=scoring["max_len"], width=scoring["width"])
        else:
            res = greedy_decode_many(model, batch, maxlen, sos, pad, **con).cpu().tolist()
        for i, r in zip(ids[:n_real], res[:n_real]):
            results[i] = r
    return results


def generate_response(model, data, corpus, vocab, maxlen=30, beam=3, penalty=2.0, nbest=5, decode_style="greedy", undisclosed_only=False,
                      ref_data=None, dialogues_per_search=0, buckets=True, sampling=None, candidates=None, no_repeat_ngram=0,
                      repetition_penalty=1.0, min_len=1, beam_groups=1, diversity_penalty=0.0, mbr=0, mbr_weights="uniform", mbr_temperature=1.0,
                      contrastive=None):
    """Decode every QA of ``data`` (data_handler.load) and return the reference's result dict, logging the reference's
    QS / REF / HYP lines per QA.  decode_style "score" generates nothing: every QA's ``candidates`` (load_candidates' ``spec``; its
    own answer without one) are scored and logged as CAND lines, best first; the answer is the best-scoring candidate, every turn
    gains "scores" in input order, and the corpus perplexity and ranking metrics (score_metrics) are logged at the end.  Candidates
    are scored whole: ``maxlen`` does not cut them.  ``no_repeat_ngram`` / ``repetition_penalty`` / ``min_len``: as decode_searches
    (a scoring run takes no constraints: ValueError).  ``beam_groups`` / ``diversity_penalty``: diverse beam search, for decode_style
    "beam_search" alone (any other style with groups > 1 or a penalty > 0: ValueError); the n-best lines and the result are as for the
    plain beam search, and so is the number of dialogues per search.  ``mbr`` = N in 1..4 (decode_style "beam_search" or "sample";
    ValueError elsewhere): minimum-Bayes-risk selection — the HYP lines come in its order, so HYP[1] is the answer, one line
    "MBR: e_1 e_2 ..." (the expected utilities, in that order) follows them, and every turn gains "mbr"; ``mbr_weights`` "uniform" or
    "score" with ``mbr_temperature`` > 0 (decode.mbr_rerank).  decode_style "contrastive" (``contrastive``: dict(k, alpha), defaults 5 and
    0.6; decode.contrastive_decode_many): one answer per QA, logged as greedy's HYP line; every turn gains "contrastive" — its score and,
    per chosen token (<eos> included), the log-probability, degeneration penalty and rank.  The search is k rows wide on the
    launch-per-sublayer pass; it takes ``min_len`` but no Ensemble, mbr, row constraints or candidates, and — as every style but beam_search —
    no beam_groups / diversity_penalty (ValueError each)."""
    if not 0 <= int(mbr) <= 4 or mbr_weights not in ("uniform", "score") or not mbr_temperature > 0:
        raise ValueError("generate_response: mbr in 0..4, mbr_weights 'uniform' or 'score', mbr_temperature > 0")
    if mbr and decode_style not in ("beam_search", "sample"):
        raise ValueError("generate_response: mbr selects among several hypotheses: decode_style beam_search or sample")
    if mbr and (maxlen > MBR_MAX_LEN or (decode_style == "beam_search" and nbest > MBR_MAX_HYP)):
        raise ValueError("generate_response: mbr takes at most %d hypotheses of at most %d tokens" % (MBR_MAX_HYP, MBR_MAX_LEN))
    if decode_style == "score" and (no_repeat_ngram != 0 or repetition_penalty != 1.0):
        raise ValueError("generate_response: no_repeat_ngram / repetition_penalty constrain a search; a scoring run has none")
    if decode_style == "contrastive":
        from .decode import Ensemble, _contrastive
        contrastive = dict(dict(k=5, alpha=0.6), **(contrastive or {}))
        _contrastive(contrastive["k"], contrastive["alpha"])
        if isinstance(model, Ensemble) or mbr or no_repeat_ngram != 0 or repetition_penalty != 1.0 or candidates is not None:
            raise ValueError("generate_response: decode_style contrastive takes one model and no mbr, no_repeat_ngram, repetition_penalty or candidates")
    if decode_style == "beam_search":
        from .decode import _diverse
        _diverse(beam, beam_groups, diversity_penalty)
    elif beam_groups != 1 or diversity_penalty != 0:
        raise ValueError("generate_response: beam_groups / diversity_penalty go with decode_style beam_search")
    vocablist = sorted(vocab.keys(), key=lambda s: vocab[s])
    eos = vocab["<eos>"]
    lens = qa_lengths(data)
    if decode_style == "sample":
        sampling = dict(dict(samples=1, temperature=1.0, top_k=0, top_p=1.0, seed=1), **(sampling or {}))
    width = beam if decode_style == "beam_search" else (sampling["samples"] if decode_style == "sample" else 1)
    if decode_style == "contrastive":
        width = contrastive["k"]
    cands = scoring = None
    if decode_style == "score":
        cands = load_candidates(candidates, data["original"], vocab, undisclosed_only, ref_data)
        assert len(cands) == len(lens)
        # one pass shape for the whole run: the longest candidate + <eos> rounded up to 8 positions, the most candidates of a QA (<= 32) rows
        longest = max(len(t) for c in cands for t in c["tokens"])
        scoring = dict(tokens=[c["tokens"] for c in cands], max_len=_up(longest + 1, 8), width=min(32, max(len(c["tokens"]) for c in cands)))
    if dialogues_per_search > 0:
        per = dialogues_per_search
    elif decode_style in ("score", "contrastive"):
        per = LAUNCH_PASS_D              # (scoring and contrastive search run on the launch-per-sublayer pass)
    else:
        per = lambda shape: auto_dialogues(model, corpus.device, shape, maxlen, width)
    searches = plan_searches(lens, per, buckets=buckets)
    n_buckets = len({(tuple(s[2][0]),) + tuple(s[2][1:]) for s in searches})
    logging.info("%d QAs in %d searches over %d padded shapes", len(lens), len(searches), n_buckets)
    vids = {it[1]: it[0] for it in data["dialogs"]}
    mbr_kw = dict(mbr=int(mbr), mbr_weights=mbr_weights, mbr_temperature=float(mbr_temperature)) if mbr else {}
    res = decode_searches(model, corpus, searches, vids, vocab, decode_style, maxlen, beam, penalty, nbest, sampling=sampling,
                          scoring=scoring, no_repeat_ngram=no_repeat_ngram, repetition_penalty=repetition_penalty, min_len=min_len,
                          beam_groups=beam_groups, diversity_penalty=diversity_penalty, **mbr_kw,
                          **(dict(contrastive=contrastive) if decode_style == "contrastive" else {}))
    answers = []
    scores = [] if decode_style == "score" else None
    mbr_out = [] if mbr else None
    cs_out = [] if decode_style == "contrastive" else None
    qa_id = 0
    for idx, dialog in enumerate(data["original"]["dialogs"]):
        vid = dialog["image_id"]
        out = dialog["dialog"][-1:] if undisclosed_only else dialog["dialog"]
        ref = None
        if undisclosed_only and ref_data is not None:
            rd = ref_data["dialogs"][idx]
            assert rd["image_id"] == vid
            ref = rd["dialog"][-1:]
        for t, qa in enumerate(out):
            logging.info("%d %s_%d" % (qa_id, vid, t))
            logging.info("QS: " + qa["question"])
            logging.info("REF: " + (ref[t]["answer"] if ref is not None else qa["answer"]))
            r = res[qa_id]
            if decode_style == "score":
                texts = cands[qa_id]["texts"]
                order = candidate_order([c["score"] for c in r])
                for n, j in enumerate(order):
                    logging.info("CAND[%d]: %s  ( %f, %f, %d )" % (n + 1, texts[j], r[j]["score"], r[j]["logp"], r[j]["n_tokens"]))
                hyp = texts[order[0]]
                scores.append([dict(candidate=texts[j], score=c["score"], logp=c["logp"], n_tokens=c["n_tokens"]) for j, c in enumerate(r)])
            elif decode_style in ("beam_search", "sample"):
                pred_out = r[0] if decode_style == "beam_search" else r          # (sample: every draw is logged, best first)
                hyp = ""
                shown = []
                for n in range(min(nbest, len(pred_out)) if decode_style == "beam_search" else len(pred_out)):
                    hypstr = detokenize(pred_out[n][0], vocablist, eos)
                    logging.info("HYP[%d]: %s  ( %f )" % (n + 1, hypstr, pred_out[n][1]))
                    if n == 0:
                        hyp = hypstr
                    if mbr:
                        shown.append(dict(hypothesis=hypstr, score=pred_out[n][1], expected=pred_out[n][2]))
                if mbr:
                    logging.info("MBR: " + " ".join(repr(h["expected"]) for h in shown))
                    mbr_out.append(shown)
            elif decode_style == "contrastive":
                hyp = detokenize(r[0], vocablist, eos)
                logging.info("HYP: {}".format(hyp))
                cs_out.append(dict(score=r[1], logp=r[2], penalty=r[3], rank=r[4]))
            else:
                hyp = greedy_text(r, vocablist, eos)
                logging.info("HYP: {}".format(hyp))
            answers.append(hyp)
            logging.info("-----------------------")
            qa_id += 1
    if decode_style == "score":
        m = score_metrics([dict(score=[c["score"] for c in res[i]], logp=[c["logp"] for c in res[i]], n_tokens=[c["n_tokens"] for c in res[i]],
                                gt_index=cands[i]["gt_index"], ranked=cands[i]["ranked"]) for i in range(len(cands))])
        if m["perplexity"] is not None:
            logging.info("perplexity = %.10g  ( %d answers, %d tokens incl. <eos> )" % (m["perplexity"], m["n_answers"], m["n_tokens"]))
        if m["n_ranked"]:
            logging.info("MRR = %.6f  R@1 = %.6f  R@5 = %.6f  R@10 = %.6f  mean rank = %.4f  ( %d QAs with gt_index )"
                         % (m["mrr"], m["r1"], m["r5"], m["r10"], m["mean_rank"], m["n_ranked"]))
    return build_result(data["original"], undisclosed_only, answers, scores, mbr_out, cs_out)


def evaluate_result(result, reference, last=False, stopwords=""):
    """--evaluate: the answers of ``result`` (build_result's dict) scored against ``reference`` (a labelled dialogue dict; ``last``: its last
    answers, for an undisclosed-only result) by mtn_amd.evaluate on the device.  Logs the six '%s: %.3f' lines and returns what becomes the
    result JSON's top-level "eval"."""
    from . import evaluate as E
    sw = E.StopwordFilter(stopwords) if stopwords else None
    _, res = E.score_files(result, reference, last=last, stopwords=sw)
    for line in E.format_lines(res):
        logging.info(line)
    return E.summary(res)


def write_result(args, result, original, labeled_test=None):
    """The tail of a run: with --evaluate the scores (logged, and the result's "eval"), then the result JSON where --output names one."""
    if args.evaluate:
        undisclosed = bool(args.undisclosed_only)
        result["eval"] = evaluate_result(result, labeled_test if undisclosed else original, last=undisclosed, stopwords=args.stopwords)
    if args.output:
        logging.info("writing results to " + args.output)
        with open(args.output, "w") as f:
            json.dump(result, f, indent=4)
    return result


def main(argv=None):
    args = parse(argv)
    for arg in vars(args):
        if arg in ("contrastive_k", "contrastive_alpha") and args.decode_style != "contrastive":
            continue                                                        # (a run of another style prints what it always did)
        if args.evaluate or arg not in ("evaluate", "stopwords"):           # (a run without --evaluate prints what it always did)
            print("{}={}".format(arg, getattr(args, arg)))
    logging.basicConfig(level=logging.DEBUG if args.verbose >= 1 else logging.INFO, format="%(asctime)s %(levelname)s: %(message)s")
    import torch
    from . import data_handler as dh
    from . import lib
    if not torch.cuda.is_available():
        raise SystemExit("generate: the decode path runs on the GPU (HIP kernels); no GPU is available")
    lib.load()
    dev = torch.device("cuda", 0)                     # (as generate.py:133: --gpu is accepted and not used)
    torch.cuda.set_device(dev)
    logging.info("Loading model params from " + args.model)
    if args.ensemble_model:                           # every member's conf first: a mismatch ends the run before anything is loaded
        member_confs = load_ensemble_confs(args.model_conf, args.ensemble_model, args.ensemble_conf)
        vocab, train_args = member_confs[0]
    else:
        vocab, train_args = load_conf(args.model_conf)
    state = load_state_dict(args.model + ".pth.tar")
    logging.info("#vocab = %d" % len(vocab))
    logging.info("Loading test data from " + args.test_set)
    test_data = dh.load(train_args.fea_type, args.test_path, args.test_set, vocab=vocab, include_caption=train_args.include_caption,
                        separate_caption=bool(train_args.separate_caption), max_history_length=train_args.max_history_length,
                        merge_source=bool(train_args.merge_source), undisclosed_only=args.undisclosed_only)
    if not (len(test_data["dialogs"]) and len(test_data["dialogs"][0]) > 6):
        raise SystemExit("generate: the model needs the caption as its own stream (a conf with separate_caption 1 and include_caption "
                         "caption|summary|caption,summary, as run.sh trains it)")
    if not args.ensemble_model:
        model = build_model(vocab, train_args, dh.feature_shape(test_data), state, args.compute_dtype, dev)
    else:
        # a member at weight 0 takes no part in the combination (decode.Ensemble never runs it): it is not built at all
        from .decode import Ensemble
        prefixes = [args.model] + list(args.ensemble_model)
        weights = list(args.ensemble_weights) if args.ensemble_weights is not None else [1.0] * len(prefixes)
        members = []
        for k, (prefix, (_, member_args), w) in enumerate(zip(prefixes, member_confs, weights)):
            if w == 0:
                logging.info("ensemble: %s has weight 0 and is not loaded" % prefix)
                continue
            if k > 0:
                logging.info("Loading model params from " + prefix)
            sd = state if k == 0 else load_state_dict(prefix + ".pth.tar")
            members.append(build_model(vocab, member_args, dh.feature_shape(test_data), sd, args.compute_dtype, dev))
        model = Ensemble(members, [w for w in weights if w != 0], args.ensemble_mode)
        logging.info("ensemble of %d members, mode %s, weights %s" % (len(members), model.mode, " ".join("%.6g" % w for w in model.weights)))
    corpus = dh.DeviceCorpus(test_data, dev)
    logging.info("#test sample = %d" % len(test_data["dialogs"]))
    logging.info("-----------------------generate--------------------------")
    labeled_test = None
    if args.undisclosed_only and args.labeled_test is not None:
        with open(args.labeled_test, "r") as f:
            labeled_test = json.load(f)
    start_time = time.time()
    result = generate_response(model, test_data, corpus, vocab, maxlen=args.maxlen, beam=args.beam, penalty=args.penalty, nbest=args.nbest,
                               decode_style=args.decode_style, undisclosed_only=args.undisclosed_only, ref_data=labeled_test,
                               dialogues_per_search=args.dialogues_per_search, buckets=not args.no_buckets,
                               sampling=dict(samples=args.samples, temperature=args.temperature, top_k=args.top_k, top_p=args.top_p,
                                             seed=args.sample_seed), candidates=args.candidates,
                               no_repeat_ngram=args.no_repeat_ngram, repetition_penalty=args.repetition_penalty, min_len=args.min_length,
                               beam_groups=args.beam_groups, diversity_penalty=args.diversity_penalty, mbr=args.mbr,
                               mbr_weights=args.mbr_weights, mbr_temperature=args.mbr_temperature,
                               **(dict(contrastive=dict(k=args.contrastive_k, alpha=args.contrastive_alpha)) if args.decode_style == "contrastive" else {}))
    wall = time.time() - start_time
    n_qa = len(test_data["dialogs"])
    logging.info("----------------")
    logging.info("wall time = %f" % wall)
    logging.info("%d QAs, %.1f QA/s" % (n_qa, n_qa / max(wall, 1e-9)))
    write_result(args, result, test_data["original"], labeled_test)
    logging.info("done")
    return result


if __name__ == "__main__":
    main()
