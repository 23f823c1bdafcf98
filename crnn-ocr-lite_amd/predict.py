#!/usr/bin/env python3
"""Prediction CLI with the reference's flag surface (predict.py:62-79): forward on the GPU, whole-batch
HIP beam-search decode (beam_width=10, top_paths=1, merge_repeated as TF 1.8), optional edit-distance report
and prediction.csv.  --device_score (with --validate) keeps decoding and scoring on the GPU: same report, same prediction.csv.
--confusions [K] (with --validate) aligns every prediction to its truth and adds the totals of matches, substitutions, deletions and insertions
and the K (default 20) most frequent character confusions to the report, and writes confusions.csv (truth, predicted, count of every non-zero
cell) next to prediction.csv; with --device_score on the GPU (crnn_edit_ops), else on the host (metrics.confusion_matrix): same lines, same file.
--lexicon FILE decodes to the most probable word of a list (crnn_mi355x.lexicon) instead of the beam search.
--lexicon_shortlist K (with --lexicon) scores per image only the K words nearest in edit distance to the beam search's --lexicon_paths best paths.
--align (with --result_path) aligns every prediction to its own softmax map (crnn_mi355x.align) and writes alignment.csv: per character its frames
on the network's time axis and its log-probability.
--lm FILE decodes with a character language model in the beam search (crnn_mi355x.lm): FILE is a saved CharLM (.npz) or a word list to count one from.
--nbest K (with --result_path) also writes nbest.csv: per image the K best paths of the beam with their scores.
--detect treats every image under --image_path as a page and finds its word boxes itself (crnn_mi355x.detect: threshold, smearing, connected
components) instead of reading them from --boxes; with --device_ingest the boxes are found on the GPU, on the same upload the crops are cut from.
prediction.csv then carries every box next to its prediction.
--detect_adaptive RADIUS (with --detect) binarises every page adaptively first (Sauvola, crnn_mi355x.binarize), for unevenly lit pages; the boxes come
from the binarised page, the crops from the grey one.
--deskew (with --detect) estimates every page's skew first and rotates the page by it (crnn_mi355x.deskew: sheared projection profiles, a
fixed-point bilinear resampling); the boxes are found on, the crops cut from and the box columns of prediction.csv refer to the DESKEWED page.
Every page's candidate index and angle are printed, and saved as skew.csv next to prediction.csv."""
import argparse
import os
import pickle
import re
import time

import numpy as np
from numpy.random import RandomState


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('--model_path', type=str, required=True)
    parser.add_argument('--image_path', type=str, required=True)
    parser.add_argument('--result_path', type=str, required=False, default=None)
    parser.add_argument('--max_len', type=int, required=False, default=23)
    parser.add_argument('--boxes', type=str, required=False, default=None)
    parser.add_argument('--val_fname', type=str, required=False, default=None)
    parser.add_argument('--num_instances', type=int, default=None)
    parser.add_argument('--G', type=int, default=-1)
    parser.add_argument('--batch_size', type=int, default=64)
    parser.add_argument('--random_state', type=int, default=42)
    parser.add_argument('--train_portion', type=float, default=.9)
    parser.add_argument('--validate', action='store_true')
    parser.add_argument('--mjsynth', action='store_true')
    parser.add_argument('--imgh', type=int, default=100)
    parser.add_argument('--imgW', type=int, default=32)
    parser.add_argument('--workers', type=int, default=0,
                        help='image decoding processes feeding the generator (0 = the reference\'s single-threaded loader)')
    parser.add_argument('--device_ingest', action='store_true',
                        help='build the batches on the GPU: pages go up as uint8 with a box table, one kernel crops, pads and normalises')
    parser.add_argument('--device_decode', action='store_true',
                        help='with --device_ingest: decode baseline JPEG files on the GPU too (crnn_mi355x.jpeg); other files are decoded on the host as before')
    parser.add_argument('--device_score', action='store_true',
                        help='with --validate: decode and score on the GPU (one edit-distance kernel per batch); no softmax map is copied to the host')
    parser.add_argument('--confusions', type=int, nargs='?', const=20, default=None, metavar='K',
                        help='with --validate: report the totals of the edit scripts and the K (default 20) most frequent character confusions, '
                             'and write confusions.csv next to prediction.csv; with --device_score aligned and counted on the GPU')
    parser.add_argument('--lexicon', type=str, default=None,
                        help='a word list, one word per line: decode to the word of the list with the highest CTC probability instead of the beam search')
    parser.add_argument('--lexicon_shortlist', type=int, default=None,
                        help='with --lexicon: score per image only the K (1..1024) words nearest in edit distance to the beam search\'s paths (50 is a placeholder: tune it)')
    parser.add_argument('--lexicon_paths', type=int, default=None,
                        help='with --lexicon_shortlist: how many of the beam search\'s best paths (1..8, default 1) the shortlist is made from')
    parser.add_argument('--align', action='store_true',
                        help='with --result_path: also write alignment.csv -- the best CTC path of every prediction through its own softmax map, per character its frames and log-probability')
    parser.add_argument('--lm', type=str, default=None,
                        help='beam search with a character language model: a CharLM saved as .npz, or a word list (one word per line, optional tab-separated count) to count one from')
    parser.add_argument('--lm_order', type=int, default=3, help='n-gram order of a model counted from a word list')
    parser.add_argument('--lm_weight', type=float, default=0.5, help='alpha: weight of the language model\'s log-probabilities (a placeholder default: tune it)')
    parser.add_argument('--lm_bonus', type=float, default=0.0, help='beta: bonus per character (a placeholder default: tune it)')
    parser.add_argument('--nbest', type=int, default=None,
                        help='with --result_path: also write nbest.csv -- file, rank, text and score of the K best paths of the beam search')
    parser.add_argument('--detect', action='store_true',
                        help='every image under --image_path is a page: find its word boxes (threshold, run-length smearing, connected components) '
                             'instead of reading --boxes; with --device_ingest on the GPU, sharing the page upload with the crops')
    parser.add_argument('--detect_gap_x', type=int, default=None, help='with --detect: background runs up to this long inside a row are bridged, 0..64 (the default is a placeholder: tune it)')
    parser.add_argument('--detect_gap_y', type=int, default=None, help='with --detect: the same down the columns, 0..16 (a placeholder default: tune it)')
    parser.add_argument('--detect_min_w', type=int, default=None, help='with --detect: narrowest box kept (a placeholder default: tune it)')
    parser.add_argument('--detect_min_h', type=int, default=None, help='with --detect: lowest box kept (a placeholder default: tune it)')
    parser.add_argument('--detect_min_ink', type=int, default=None, help='with --detect: fewest ink pixels of a box kept (a placeholder default: tune it)')
    parser.add_argument('--detect_threshold', type=int, default=None, help='with --detect: ink threshold 0..254, or -1 for Otsu per page (the default)')
    parser.add_argument('--detect_cap', type=int, default=None, help='with --detect: most boxes kept per page (default 1024)')
    parser.add_argument('--detect_adaptive', type=int, default=None, metavar='RADIUS',
                        help='with --detect: binarise every page adaptively first (Sauvola, crnn_mi355x.binarize) over windows of 2 RADIUS + 1 pixels, '
                             'RADIUS 1..31 (15 is a placeholder: tune it), for unevenly lit pages; it takes the place of --detect_threshold. '
                             'Only the boxes come from the binarised page: the crops are cut from the original grey page, which is what the recogniser was trained on')
    parser.add_argument('--detect_adaptive_k', type=float, default=None, metavar='K',
                        help='with --detect_adaptive: Sauvola\'s k, used as round(K * 256) / 256 in 0..255/256 (the default 0.2 is a placeholder: tune it)')
    parser.add_argument('--deskew', action='store_true',
                        help='with --detect: estimate every page\'s skew (sheared projection profiles) and rotate the page by it before the boxes are '
                             'found; boxes and crops then refer to the deskewed page.  With --device_ingest on the GPU, in a second arena')
    parser.add_argument('--deskew_steps', type=int, default=None, metavar='N',
                        help='with --deskew: the candidates are the slopes a * Q / 65536 for a = -N..N, N 0..64 (48 is a placeholder: tune it)')
    parser.add_argument('--deskew_slope_step', type=int, default=None, metavar='Q',
                        help='with --deskew: the distance Q / 65536 between two candidate slopes, Q 1..1024 with N * Q <= 16384 (256 is a placeholder: tune it)')
    return parser


PAGES_PER_UPLOAD = 16                                        # --detect --device_ingest: pages per arena
DETECT_CAP = 1024                                            # crnn_mi355x.detect.DEFAULTS["cap"]: the host path keeps what the device keeps
DETECT_FLAGS = ("gap_x", "gap_y", "min_w", "min_h", "min_ink", "threshold", "cap")


def detect_params(args):
    """The --detect_* flags that were given -> keyword arguments of detect_words_host / WordDetector."""
    p = {k: getattr(args, "detect_" + k) for k in DETECT_FLAGS if getattr(args, "detect_" + k) is not None}
    if args.detect_adaptive is not None:
        p["adaptive"] = dict(radius=args.detect_adaptive, **({} if args.detect_adaptive_k is None else {"k": args.detect_adaptive_k}))
    elif args.detect_adaptive_k is not None:
        p["adaptive"] = dict(k=args.detect_adaptive_k)       # (parse_args refuses it: k tunes --detect_adaptive)
    return p


def deskew_params(args):
    """--deskew and its flags -> keyword arguments of deskew_host / Deskewer (the ink is the detector's: its threshold or its adaptive
    binarisation), or None without --deskew."""
    if not args.deskew:
        return None
    p = {k: getattr(args, "deskew_" + k) for k in ("steps", "slope_step") if getattr(args, "deskew_" + k) is not None}
    given = detect_params(args)
    p.update({k: given[k] for k in ("threshold", "adaptive") if k in given})
    return p


def parse_args(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.device_score and not args.validate:
        parser.error("--device_score scores against the truth: it needs --validate")
    if args.confusions is not None and not args.validate:
        parser.error("--confusions aligns the predictions to the truth: it needs --validate")
    if args.confusions is not None and args.confusions < 0:
        parser.error("--confusions must be 0 or more")
    if args.align and args.result_path is None:
        parser.error("--align writes alignment.csv next to prediction.csv: it needs --result_path")
    if args.align and args.device_score:
        parser.error("--align reads the softmax maps, which --device_score never materialises: use one or the other")
    if args.lm is not None and args.lexicon is not None:
        parser.error("--lm and --lexicon are two decoders: use one or the other")
    if (args.lexicon_shortlist is not None or args.lexicon_paths is not None) and args.lexicon is None:
        parser.error("--lexicon_shortlist and --lexicon_paths shorten a word list: they need --lexicon")
    if args.lexicon_paths is not None and args.lexicon_shortlist is None:
        parser.error("--lexicon_paths chooses the paths a shortlist is made from: it needs --lexicon_shortlist")
    if args.lexicon_shortlist is not None and not 1 <= args.lexicon_shortlist <= 1024:
        parser.error("--lexicon_shortlist must be 1..1024")
    if args.lexicon_paths is not None and not 1 <= args.lexicon_paths <= 8:
        parser.error("--lexicon_paths must be 1..8")
    if args.nbest is not None and args.result_path is None:
        parser.error("--nbest writes nbest.csv next to prediction.csv: it needs --result_path")
    if args.nbest is not None and args.lexicon is not None:
        parser.error("--nbest lists paths of the beam search: it does not go with --lexicon")
    if args.nbest is not None and args.device_score:
        parser.error("--nbest reads the softmax maps, which --device_score never materialises: use one or the other")
    if args.nbest is not None and not 1 <= args.nbest <= 64:
        parser.error("--nbest must be 1..64")
    if args.detect and args.boxes is not None:
        parser.error("--detect finds the boxes, --boxes reads them: use one or the other")
    if args.detect and args.validate:
        parser.error("--detect has no truth to validate against: it does not go with --validate")
    if not args.detect and detect_params(args):
        parser.error("the --detect_* flags tune --detect: they need it")
    if args.detect_adaptive_k is not None and args.detect_adaptive is None:
        parser.error("--detect_adaptive_k tunes --detect_adaptive: it needs it")
    if args.deskew and not args.detect:
        parser.error("--deskew straightens the pages --detect reads: it needs --detect")
    if (args.deskew_steps is not None or args.deskew_slope_step is not None) and not args.deskew:
        parser.error("--deskew_steps and --deskew_slope_step tune --deskew: they need it")
    if args.deskew:
        from crnn_mi355x import deskew
        try:
            deskew.check_params(**{k: v for k, v in deskew_params(args).items() if k in ("steps", "slope_step")})
        except ValueError as e:
            parser.error(str(e))
    if args.detect:
        from crnn_mi355x.detect import adaptive_setup, check_params, DEFAULTS
        try:
            given = detect_params(args)
            adaptive_setup(given.pop("adaptive", None), given.get("threshold", DEFAULTS["threshold"]), DEFAULTS["polarity"])
            check_params(dict(DEFAULTS, **given))
        except ValueError as e:
            parser.error(str(e))
    return args


def detect_on_device(args, names, model, img_size, U):
    """--detect --device_ingest: groups of pages go up once; the detector finds the boxes in the arena and the crops are cut from the same
    arena, batch by batch -> ({page: boxes}, softmax maps of every box in order, {page: skew index} or None).  Pages without boxes are left
    out.  With --detect_adaptive the detector binarises the arena into a second one and finds the boxes there; the crops still come from the
    grey arena uploaded here.  With --deskew every uploaded arena is deskewed into a second one first (Deskewer.run): the boxes are found in
    and the crops cut from that one."""
    det = U.WordDetector(**detect_params(args))
    ing = U.DeviceIngest(img_size, normed=True)
    deskewer = U.Deskewer(**deskew_params(args)) if args.deskew else None
    bboxs, maps, skew = {}, [], ({} if args.deskew else None)

    def flush(group):
        pages = [U.read_img(n) for n in group]
        arena = ing.upload(pages)
        if deskewer is not None:
            arena = deskewer.run(None, arena=arena)              # boxes and crops refer to the deskewed pages from here on
            skew.update(zip(group, arena.index.cpu().tolist()))
        index, rects = [], []
        for k, (name, boxes) in enumerate(zip(group, det.boxes(None, arena=arena))):
            if boxes:
                bboxs[name] = boxes
                index += [k] * len(boxes)
                rects += [U.box_slices(b, pages[k].shape) for b in boxes]
        for i in range(0, len(index), args.batch_size):
            part = slice(i, i + args.batch_size)
            x = ing.crops(None, index[part], rects[part], ing.plan(rects[part]), batch=args.batch_size, arena=arena)
            maps.append(model.predict_on_batch(x)[:len(index[part])])
    for i in range(0, len(names), PAGES_PER_UPLOAD):
        flush(names[i:i + PAGES_PER_UPLOAD])
    return bboxs, (np.concatenate(maps, 0) if maps else None), skew


def detect_on_host_deskewed(args, names, model, reader, img_size, U):
    """--detect --deskew without --device_ingest: every page goes through deskew_host, the boxes are found on its result and the crops are
    cut from its result (the reader would cut them from the file) -> ({page: boxes}, softmax maps of every box in order, {page: skew index})."""
    bboxs, crops, skew = {}, [], {}
    for name in names:
        flat, skew[name] = U.deskew_host(U.read_img(name), **deskew_params(args))
        rects, _ = U.detect_words_host(flat, **dict({"cap": DETECT_CAP}, **detect_params(args)))
        if len(rects):
            bboxs[name] = [(None, int(r[0]), int(r[2]), int(r[1]), int(r[3])) for r in rects[U.reading_order(rects)]]
            for b in bboxs[name]:
                pixels, _ = U.open_img(flat[b[1]:b[3], b[2]:b[4]], img_size, p=0.)
                crops.append((U.norm(pixels, reader.mean, reader.std) if reader.normed else pixels)[:, :, np.newaxis])
    maps = []
    for i in range(0, len(crops), args.batch_size):
        x = np.zeros((args.batch_size,) + tuple(img_size))
        x[:len(crops[i:i + args.batch_size])] = np.stack(crops[i:i + args.batch_size])
        maps.append(model.predict_on_batch(x)[:len(crops[i:i + args.batch_size])])
    return bboxs, (np.concatenate(maps, 0) if maps else None), skew


def main(argv=None):
    args = parse_args(argv)
    if args.G >= 0:
        os.environ.setdefault("HIP_VISIBLE_DEVICES", str(args.G))   # the reference falls back to CPU for G<0; this build has no CPU path
    import utils as U

    prng = RandomState(args.random_state)
    model = U.init_predictor(U.load_custom_model(args.model_path, model_name='/model.json', weights="/final_weights.h5"))
    classes = {ch: i for i, ch in enumerate(U.get_lexicon())}
    inverse_classes = {v: k for k, v in classes.items()}
    decoder = U.DecodeCTCPred(top_paths=1, beam_width=10, inverse_classes=inverse_classes)
    if args.lexicon is not None:
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                  # the count is printed below instead
            lexicon = U.Lexicon([line.rstrip("\r\n") for line in open(args.lexicon)], inverse_classes)
        mode = "every word scored" if args.lexicon_shortlist is None else \
            "shortlist of the %d words nearest to %d beam path(s)" % (args.lexicon_shortlist, args.lexicon_paths or 1)
        print(" [INFO] Lexicon: %d words, %d rejected (a character outside the alphabet, or longer than 31); %s "
              % (len(lexicon), len(lexicon.rejected), mode))
        decoder = U.LexiconDecoder(lexicon, top_paths=1, shortlist=args.lexicon_shortlist, paths=args.lexicon_paths or 1)
    if args.lm is not None or args.nbest is not None:
        lm = None
        if args.lm is not None and args.lm.endswith(".npz"):
            lm = U.CharLM.load(args.lm)
        elif args.lm is not None:
            from crnn_mi355x.lm import read_word_list
            words, counts = read_word_list(args.lm)
            lm = U.CharLM.from_words(words, inverse_classes, order=args.lm_order, counts=counts)
            print(" [INFO] Language model: order %d from %d words, %d rejected (a character outside the alphabet) " % (lm.order, len(words), len(lm.rejected)))
        # without --lm this is the beam search above (merge_repeated as TF) with its other paths kept
        decoder = U.LMDecoder(lm, alpha=args.lm_weight, beta=args.lm_bonus, beam_width=max(10, args.nbest or 1), top_paths=args.nbest or 1,
                              merge_repeated=lm is None, inverse_classes=inverse_classes)
    img_size = (args.imgh, args.imgW, 1)

    def walk():
        return np.array([os.path.join(dp, f) for dp, dn, fs in os.walk(args.image_path) for f in fs if re.search('png|jpeg|jpg', f)])

    if args.validate and args.mjsynth:
        fnames = np.array(U.parse_mjsynth(args.image_path, open(os.path.join(args.image_path, args.val_fname)).readlines()))
    else:
        fnames = walk()
        if args.validate:
            prng.shuffle(fnames)
            fnames = fnames[int(len(fnames) * args.train_portion):]
    if args.num_instances is not None:
        fnames = fnames[np.random.randint(0, len(fnames), min(args.num_instances, len(fnames)))]
    if args.device_decode and not args.device_ingest:
        raise SystemExit("--device_decode goes with --device_ingest")
    if args.device_ingest:
        reader = U.DeviceReadf(img_size=img_size, normed=True, batch_size=args.batch_size, transform_p=0., classes=classes, max_len=args.max_len, workers=args.workers,
                               device_decode=args.device_decode)
    else:
        reader = U.Readf(img_size=img_size, normed=True, batch_size=args.batch_size, transform_p=0., classes=classes, max_len=args.max_len, workers=args.workers)
    length = len(fnames)
    bboxs = {}
    predicted = None
    skew = None
    if args.detect:
        fnames = sorted(str(f) for f in walk())                   # every image is a page; no halving of the page set
        if args.device_ingest:
            bboxs, predicted, skew = detect_on_device(args, fnames, model, img_size, U)
        elif args.deskew:
            bboxs, predicted, skew = detect_on_host_deskewed(args, fnames, model, reader, img_size, U)
        else:
            for name in fnames:
                rects, _ = U.detect_words_host(U.read_img(name), **dict({"cap": DETECT_CAP}, **detect_params(args)))
                if len(rects):
                    bboxs[name] = [(None, int(r[0]), int(r[2]), int(r[1]), int(r[3])) for r in rects[U.reading_order(rects)]]
        if skew is not None:
            from crnn_mi355x.deskew import DEFAULTS as DESKEW_DEFAULTS, angle_of
            q = args.deskew_slope_step if args.deskew_slope_step is not None else DESKEW_DEFAULTS["slope_step"]
            skew = [(f, skew[f], angle_of(skew[f], q)) for f in fnames]
            for f, a, deg in skew:
                print(" [INFO] Skew of %s: index %d, %.2f degrees " % (os.path.basename(f), a, deg))
        empty = [f for f in fnames if f not in bboxs]
        if empty:
            print(" [INFO] %d page(s) without a word box left out: %s " % (len(empty), ", ".join(os.path.basename(f) for f in empty[:5])))
        if not bboxs:
            raise SystemExit(" [ERROR] --detect found no word box on any of the %d pages" % len(fnames))
        length = sum(len(v) for v in bboxs.values())
        fnames = [f for f in fnames if f in bboxs]
        print(" [INFO] Detected %d word boxes on %d pages " % (length, len(fnames)))
    elif args.boxes is not None:
        bboxs = pickle.load(open(args.boxes, "rb"))          # {image: [(word|None, x0, y0, x1, y1), ...]}
        half = len(bboxs) // 2
        bboxs = {os.path.join(args.image_path, k): v for i, (k, v) in enumerate(bboxs.items()) if i <= half}
        length = sum(len(v) for v in bboxs.values())
        fnames = list(bboxs.keys())
        if args.validate:
            y_true = np.array([reader.make_target(el[0]) for v in bboxs.values() for el in v], dtype=object)
    elif not args.detect:
        y_true = reader.get_labels(fnames)
    steps = -(-length // args.batch_size)
    print(" [INFO] Predicting... ")
    start = time.time()
    score = None
    if args.device_score:                                    # forward, beam search and edit distance per batch, all on the device
        score = model.score_generator(reader.run_generator(fnames, bboxs=bboxs, downsample_factor=2), steps=steps, decoder=decoder, length=length,
                                      confusions=args.confusions is not None)
        print(" [INFO] %d images processed in %s sec. " % (len(fnames), round(time.time() - start, 2)))
        start = time.time()
        predicted_text = score.texts(decoder)
        print(" [INFO] %d predictions decoded in %s sec. " % (steps * args.batch_size, round(time.time() - start, 2)))
    else:
        if predicted is None:                                # (--detect --device_ingest made the maps on the upload it found the boxes in)
            predicted = model.predict_generator(reader.run_generator(fnames, bboxs=bboxs, downsample_factor=2), steps=steps)
        print(" [INFO] %d images processed in %s sec. " % (len(fnames), round(time.time() - start, 2)))
        start = time.time()
        predicted_text = decoder.decode(predicted)[:length]
        print(" [INFO] %d predictions decoded in %s sec. " % (len(predicted), round(time.time() - start, 2)))
    if args.result_path is not None:
        import pandas as pd
        if len(fnames) != len(predicted_text):
            fnames = [f for f in bboxs for _ in range(len(bboxs[f]))]
        out_name = os.path.join(args.result_path, "prediction.csv")
        table = {"fname": fnames, "prediction": predicted_text}
        if args.detect:                                      # the box of every row, as page[r0:r1, c0:c1]
            flat = [b for f in bboxs for b in bboxs[f]]
            table.update(r0=[b[1] for b in flat], c0=[b[2] for b in flat], r1=[b[3] for b in flat], c1=[b[4] for b in flat])
        pd.DataFrame(table).to_csv(out_name)
        print(" [INFO] Prediction example: \n", predicted_text[:10])
        print(" [INFO] Result store in: ", out_name)
        if skew is not None:                                 # the boxes above refer to the pages rotated by these angles
            pd.DataFrame(skew, columns=["fname", "index", "degrees"]).to_csv(os.path.join(args.result_path, "skew.csv"))
        if args.nbest is not None:
            nbest = decoder.decode_topk(predicted[:length])
            pd.DataFrame([{"fname": f, "rank": k, "text": t, "score": v} for f, paths in zip(fnames, nbest) for k, (t, v) in enumerate(paths)],
                         columns=["fname", "rank", "text", "score"]).to_csv(os.path.join(args.result_path, "nbest.csv"))
        if args.align:
            from crnn_mi355x.align import CTCAligner, write_alignment_csv
            aligned = CTCAligner(inverse_classes).align(predicted[:length], predicted_text)
            write_alignment_csv(os.path.join(args.result_path, "alignment.csv"), fnames, aligned)
    if args.validate:
        print(" [INFO] Computing edit distance metric... ")
        start = time.time()
        true_text = [decoder.labels_to_text(y_true[i]) for i in range(len(y_true))]
        print(" [INFO] Example pairs (predicted, true): \n", list(zip(predicted_text[:10], true_text[:10])))
        if score is not None:
            ed, ned = score.edit_distance, score.normalized_edit_distance
        else:
            ed = U.edit_distance(predicted_text, true_text)
            ned = U.normalized_edit_distance(predicted_text, true_text)
        print(" [INFO] edit distances calculated in %s sec. " % round(time.time() - start, 2))
        print(" [INFO] mean edit distance: %f ; normalized edit distance score: %f " % (ed, ned))
        if args.confusions is not None:
            if score is not None:                            # counted on the device, batch by batch, and read once
                confusions = score.confusions
            else:
                pairs = [([classes[c] for c in p], [classes[c] for c in t]) for p, t in zip(predicted_text, true_text)]
                confusions = U.Confusions(U.confusion_matrix(pairs, len(inverse_classes)), inverse_classes)
            print(confusions.report(args.confusions))
            if args.result_path is not None:
                confusions.to_csv(os.path.join(args.result_path, "confusions.csv"))


if __name__ == '__main__':
    main()
