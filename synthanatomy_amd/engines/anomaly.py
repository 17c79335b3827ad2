"""``run_vqvae.py --mode=anomaly``: its flags, their refusals, the stage and its score table.

``--mode=anomaly`` (MI355X-only; the rule is this project's own) is the last stage of the healing application: every ``--validation_subjects``
scan goes through the usual input path, the files ``run_transformer.py --mode=healing`` wrote for its codes (``<stem>_quantization_0_healed_sample.npy``,
``..._resampled.npy``, ``..._nll.npy``) are found by stem under ``--anomaly_codes=<dir|glob>`` (default: this experiment's outputs directory), the healed
codes are decoded and ``sa_anomaly_map`` turns scan, decoding and the latent weight grid into ``<name>_anomaly_map`` on the device, with no file in
between; ``<name>_healed_reconstruction`` is written next to it (``.npy``, or NIfTI with the source geometry under ``--output_ext``) and every rank
writes ``anomaly_scores_rank<k>.csv`` (subject, sum, max and, with ``--anomaly_labels``, Dice at the threshold, the best Dice over the 256 histogram
edges with its threshold, and the average precision).  ``--anomaly_weight=mask|nll|none`` picks the grid, ``--anomaly_sigma`` the Gaussian that smooths
its upsampling (None: half the down-sampling factor), ``--anomaly_residual=abs|positive|negative`` the sign convention, ``--anomaly_threshold`` the
operating point of the TP / FP / FN counts, ``--anomaly_hist_max`` the top of the histogram, ``--anomaly_labels`` any input spec of label volumes
(matched by stem, reoriented and cropped like the scans, never normalised, class 1 where > 0.5).

``--anomaly_ensemble=<dir|glob>,<dir|glob>[,...]`` (MI355X-only; default None: nothing changes) scores every scan against 2 to 16 healings of
its codes, one ``run_transformer.py --mode=healing`` outputs directory per ordering or seed: every spec is searched like ``--anomaly_codes`` (which it
replaces; giving both is refused), every member is decoded on its own, and ``sa_anomaly_map_ensemble`` writes the mean of the members' weighted residuals
as ``<name>_anomaly_map`` in one pass, with the scores of that mean; ``<name>_healed_reconstruction_m<k>`` is member k's decoding in flag order and
``anomaly_scores_rank<k>.csv`` gains a last column ``members``.  The other ``--anomaly_*`` flags are shared by the members.

``--anomaly_min_component=<voxels>`` (MI355X-only; default None: nothing changes) cleans the segmentation ``[map >= --anomaly_threshold]``
(which it needs) on the device: ``sa_components`` labels its connected components under ``--anomaly_connectivity=6|18|26`` (default 26), drops those
below that many voxels and counts lesions; the single map and the ensemble map both go through it.  ``<name>_anomaly_segmentation`` ({0, 1}) is
written like the map and the CSV gains ``components``, ``components_kept``, ``voxels_kept``, ``largest_component`` and, with ``--anomaly_labels``,
``dice_cleaned``, ``lesions``, ``lesions_detected``, ``lesion_recall``, ``lesion_precision``, ``lesion_f1`` (before ``members``).

``--anomaly_median=1|3|5`` and ``--anomaly_mask=scan|<dir|glob>`` (MI355X-only; default None: nothing changes) filter the map, single or
ensemble, on the device before the components: ``sa_anomaly_median`` restricts it to the mask by a select, takes the 3-D median of that side (zeros
outside the volume) and restricts it again; a mask alone means side 1.  ``scan`` is ``[x > --anomaly_mask_threshold]`` (default 0.0, only valid with
``scan``) of the scan as the encoder saw it; otherwise mask volumes are matched to the subjects by stem and loaded like ``--anomaly_labels``
(reoriented and cropped like the scan, never normalised; foreground where > 0.5).  ``--anomaly_mask_erosion=0..4`` (default 0, needs a mask) erodes the
mask that many times with the 6-neighbourhood, the outside of the volume counting as background.  ``<name>_anomaly_map`` stays the raw map,
``<name>_anomaly_map_filtered`` is written like it, ``--anomaly_min_component`` then cleans the filtered map, and the CSV keeps its columns (the raw
map's) and gains ``filtered_sum``, ``filtered_max`` and, with ``--anomaly_labels``, ``filtered_dice``, ``filtered_best_dice``,
``filtered_best_dice_threshold``, ``filtered_average_precision`` before the component columns."""
import math
import os

import numpy as np
import torch

from ..metrics.anomaly import MAX_MEMBERS, MAX_SIGMA, RESIDUALS, anomaly_map, anomaly_map_ensemble, average_precision, best_dice, dice_from_counts
from ..metrics.components import CONNECTIVITIES, connected_components, lesion_scores
from ..metrics.median import MAX_EROSION, SIZES, median_filter_map
from ..utils.general import check_for_checkpoints, list_inputs, load_network_state, log, shard_for_rank, stem
from ..utils.volumes import VolumeWriter, _batches, _load_volume

ANOMALY_FLAGS = dict(      # the stage's flags and their defaults: run_vqvae.DEFAULTS takes them in
    anomaly_codes=None, anomaly_weight="mask", anomaly_sigma=None, anomaly_residual="abs", anomaly_threshold=None, anomaly_hist_max=1.0, anomaly_labels=None,
    anomaly_ensemble=None, anomaly_min_component=None, anomaly_connectivity=26, anomaly_median=None, anomaly_mask=None, anomaly_mask_threshold=0.0, anomaly_mask_erosion=0,
)


def _off_default(value, default):
    return value is not None and (isinstance(value, bool) or value != default)


# The flags that every other mode refuses (the rest are inert there), in the order of their refusals, each with the rule that says it was given.
ANOMALY_ONLY = (("anomaly_median", _off_default), ("anomaly_mask", _off_default), ("anomaly_mask_threshold", _off_default), ("anomaly_mask_erosion", _off_default),
                ("anomaly_min_component", _off_default), ("anomaly_connectivity", lambda value, default: value != default), ("anomaly_ensemble", _off_default))


def anomaly_only_flags_given(cfg):
    return [name for name, given in ANOMALY_ONLY if given(cfg[name], ANOMALY_FLAGS[name])]


def _anomaly_sigma(cfg):
    """--anomaly_sigma, or half the largest down-sampling factor of the network the flags describe"""
    factor = math.prod(int(p[1]) for p in list(cfg["downsample_parameters"])[:int(cfg["no_levels"])])
    return cfg["anomaly_sigma"] if cfg["anomaly_sigma"] is not None else factor / 2.0


def _ensemble_specs(cfg):
    """--anomaly_ensemble as a list of specs (a comma-separated string, a tuple or a list), or None without the flag"""
    v = cfg["anomaly_ensemble"]
    return None if v is None else v.split(",") if isinstance(v, str) else list(v) if isinstance(v, (tuple, list)) else [v]


def _filtered(cfg):
    return cfg["anomaly_median"] is not None or cfg["anomaly_mask"] is not None      # DESIGN 7.18; a mask alone is size 1


def _check_anomaly_flags(cfg):
    """the --anomaly_* flags act or refuse (before anything touches the device)"""
    given = anomaly_only_flags_given(cfg)
    if given and cfg["mode"] != "anomaly":
        raise ValueError(f"--{given[0]}={cfg[given[0]]}: the flag belongs to --mode=anomaly, not --mode={cfg['mode']}")
    # --anomaly_median / --anomaly_mask / --anomaly_mask_threshold / --anomaly_mask_erosion, each by its name
    k = cfg["anomaly_median"]
    if k is not None and (isinstance(k, bool) or not isinstance(k, int) or k not in SIZES):
        raise ValueError(f"--anomaly_median={k}: choices are 1, 3 and 5 (the window's side) or None")
    mask = cfg["anomaly_mask"]
    if mask is not None and (not isinstance(mask, str) or not mask.strip()):
        raise ValueError(f"--anomaly_mask={mask}: scan, a directory or a glob is needed")
    mt = cfg["anomaly_mask_threshold"]
    if isinstance(mt, bool) or not isinstance(mt, (int, float)) or mt != mt or abs(mt) == float("inf"):
        raise ValueError(f"--anomaly_mask_threshold={mt}: a finite number is needed")
    if mt != ANOMALY_FLAGS["anomaly_mask_threshold"] and mask != "scan":
        raise ValueError(f"--anomaly_mask_threshold={mt}: the flag thresholds the scan and needs --anomaly_mask=scan (given: {mask})")
    e = cfg["anomaly_mask_erosion"]
    if isinstance(e, bool) or not isinstance(e, int) or not 0 <= e <= MAX_EROSION:
        raise ValueError(f"--anomaly_mask_erosion={e}: an integer in 0..{MAX_EROSION} is needed")
    if e > 0 and mask is None:
        raise ValueError(f"--anomaly_mask_erosion={e}: there is nothing to erode without --anomaly_mask")
    for name in given:
        if name in ("anomaly_min_component", "anomaly_connectivity") and cfg["anomaly_threshold"] is None:
            raise ValueError(f"--{name}={cfg[name]}: the components are those of [map >= --anomaly_threshold], which is not given")
    n = cfg["anomaly_min_component"]
    if n is not None and (isinstance(n, bool) or not isinstance(n, int) or n < 1 or n >= 2 ** 31 - 1):
        raise ValueError(f"--anomaly_min_component={n}: an integer >= 1 (voxels) or None is needed")
    c = cfg["anomaly_connectivity"]
    if isinstance(c, bool) or c not in CONNECTIVITIES:
        raise ValueError(f"--anomaly_connectivity={c}: choices are 6, 18 and 26")
    specs = _ensemble_specs(cfg)
    if specs is not None:
        flag = f"--anomaly_ensemble={cfg['anomaly_ensemble']}"
        for sp in specs:
            if not isinstance(sp, str):
                raise ValueError(f"{flag}: {sp!r} is not a directory or a glob (a comma-separated string or a tuple of strings is needed)")
            if not sp.strip():
                raise ValueError(f"{flag}: an empty spec (one directory or glob per member is needed)")
        if not 2 <= len(specs) <= MAX_MEMBERS:
            raise ValueError(f"{flag}: {len(specs)} members, 2 to {MAX_MEMBERS} are needed (one healing: --anomaly_codes)")
        twice = sorted({sp for sp in specs if specs.count(sp) > 1})
        if twice:
            raise ValueError(f"{flag}: {twice[0]} is given twice (every member needs its own healing outputs)")
        if cfg["anomaly_codes"] is not None:
            raise ValueError(f"{flag} with --anomaly_codes={cfg['anomaly_codes']}: the ensemble names every member's outputs itself; give one of the two")
    if cfg["anomaly_weight"] not in ("mask", "nll", "none"):
        raise ValueError(f"--anomaly_weight={cfg['anomaly_weight']}: choices are mask, nll and none")
    if cfg["anomaly_residual"] not in RESIDUALS:
        raise ValueError(f"--anomaly_residual={cfg['anomaly_residual']}: choices are abs, positive and negative")
    sigma = _anomaly_sigma(cfg)
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float)) or not 0 <= sigma <= MAX_SIGMA:
        raise ValueError(f"--anomaly_sigma={sigma}: a number in [0, {MAX_SIGMA:g}] or None (half the down-sampling factor) is needed")
    t = cfg["anomaly_threshold"]
    if t is not None and (isinstance(t, bool) or not isinstance(t, (int, float)) or t != t or abs(t) == float("inf")):
        raise ValueError(f"--anomaly_threshold={t}: a finite number or None is needed")
    hm = cfg["anomaly_hist_max"]
    if isinstance(hm, bool) or not isinstance(hm, (int, float)) or not 0 < hm < float("inf"):
        raise ValueError(f"--anomaly_hist_max={hm}: a finite number > 0 is needed")
    if cfg["anomaly_codes"] is not None and not isinstance(cfg["anomaly_codes"], str):
        raise ValueError(f"--anomaly_codes={cfg['anomaly_codes']}: a directory or a glob is needed")
    if int(cfg["no_augmented_extractions"] or 0) > 0:
        raise ValueError(f"--no_augmented_extractions={cfg['no_augmented_extractions']}: --mode=anomaly compares every scan with its own healed codes")


def find_healing_outputs(subjects, spec, weight="mask"):
    """For every subject the files ``run_transformer.save_healing`` wrote for its codes, found by stem under ``spec`` (a directory, searched recursively,
    or a glob): ``<stem>_quantization_0_healed_sample.npy`` and next to it ``..._resampled.npy`` / ``..._nll.npy`` (``weight`` = mask / nll says which
    one is needed).  One dict per subject (keys healed, resampled, nll); a subject with no match, or with more than one, is refused by name."""
    import glob
    found = set()
    for hit in ([spec] if os.path.isdir(spec) else glob.glob(spec, recursive=True)):      # a directory the glob matches is searched like one given
        if os.path.isdir(hit):
            found.update(glob.glob(os.path.join(hit, "**", "*_healed_sample.npy"), recursive=True))
        elif hit.endswith("_healed_sample.npy"):
            found.add(hit)
    found = sorted(found)
    out = []
    for s in subjects:
        want = f"{stem(s)}_quantization_0_healed_sample.npy"
        hits = [f for f in found if os.path.basename(f) == want]
        if not hits:
            raise ValueError(f"{s}: no healing output {want} under {spec} (run_transformer.py --mode=healing writes it; see --anomaly_codes)")
        if len(hits) > 1:
            raise ValueError(f"{s}: {len(hits)} healing outputs named {want} under {spec} ({', '.join(hits)}): narrow --anomaly_codes")
        base = hits[0][:-len("healed_sample.npy")]
        rec = {"healed": hits[0], "resampled": base + "resampled.npy", "nll": base + "nll.npy"}
        need = {"mask": "resampled", "nll": "nll"}.get(weight)
        if need and not os.path.exists(rec[need]):
            raise ValueError(f"{s}: {os.path.basename(rec[need])} is missing next to {hits[0]} (--anomaly_weight={weight} needs it)")
        out.append(rec)
    return out


def find_ensemble_outputs(subjects, specs, weight="mask"):
    """``find_healing_outputs`` once per member spec: a list over the members of lists over the subjects.  A subject whose two members resolve to the
    same healed file, and a member whose code grid differs in shape from member 0's, are refused by name (host only: the ``.npy`` headers are read)."""
    members = [find_healing_outputs(subjects, spec, weight) for spec in specs]
    for j, s in enumerate(subjects):
        seen = {}
        for k, recs in enumerate(members):
            real = os.path.realpath(recs[j]["healed"])
            if real in seen:
                raise ValueError(f"{s}: members {seen[real]} ({specs[seen[real]]}) and {k} ({specs[k]}) of --anomaly_ensemble resolve to the same "
                                 f"healed file {recs[j]['healed']}")
            seen[real] = k
        shapes = [np.load(recs[j]["healed"], mmap_mode="r").shape for recs in members]
        for k, shp in enumerate(shapes):
            if shp != shapes[0]:
                raise ValueError(f"{s}: member {k} ({specs[k]}) of --anomaly_ensemble has a code grid of shape {shp}, member 0 ({specs[0]}) has "
                                 f"{shapes[0]}")
    return members


def match_labels(subjects, spec, flag="anomaly_labels", what="label"):
    """the label volume of every subject, matched by stem among ``list_inputs(spec)``; a subject without exactly one is refused by name
    (``--anomaly_mask=<dir|glob>`` finds its mask volumes the same way)"""
    found = list_inputs(spec)
    out = []
    for s in subjects:
        hits = [f for f in found if stem(f) == stem(s)]
        if len(hits) != 1:
            raise ValueError(f"{s}: {len(hits)} {what} volumes with the stem {stem(s)} in --{flag}={spec} (exactly one is needed)")
        out.append(hits[0])
    return out


def _summary_cells(s, j):
    return [repr(float(s["sum"][j])), repr(float(s["max"][j]))]


def _summary_label_cells(s, j):      # dice: "" without --anomaly_threshold, nothing was counted
    bd, bt = best_dice(s["hist"][j, 0], s["hist"][j, 1], s["inv_bin"])
    dice = "" if s["tp"] is None else repr(dice_from_counts(s["tp"][j], s["fp"][j], s["fn"][j]))
    return [dice, repr(bd), repr(bt), repr(average_precision(s["hist"][j, 0], s["hist"][j, 1]))]


def _component_cells(s, j):
    return [str(int(s[key][j])) for key in COMPONENTS[0]]


def _component_label_cells(s, j):
    rc, pr, f1 = lesion_scores(s["lesions"][j], s["lesions_detected"][j], s["components_kept"][j], s["kept_true"][j])
    return [repr(dice_from_counts(s["tp"][j], s["fp"][j], s["fn"][j])), str(int(s["lesions"][j])), str(int(s["lesions_detected"][j])), repr(rc), repr(pr), repr(f1)]


# The score table of anomaly_scores_rank<k>.csv, one definition for the header and for every row: (columns, their cells for subject j from the host summaries of one map or of its components); the *_LABELLED groups come with --anomaly_labels
SUMMARY = (("sum", "max"), _summary_cells)
SUMMARY_LABELLED = (("dice", "best_dice", "best_dice_threshold", "average_precision"), _summary_label_cells)
COMPONENTS = (("components", "components_kept", "voxels_kept", "largest_component"), _component_cells)
COMPONENTS_LABELLED = (("dice_cleaned", "lesions", "lesions_detected", "lesion_recall", "lesion_precision", "lesion_f1"), _component_label_cells)


def score_table(cfg):
    """[(columns, which summaries they read: "raw" / "filtered" / "components", cells)] in the CSV's order, from the flags alone (a rank without subjects
    still writes the header): the raw map's summary groups, the same with ``filtered_`` for the filtered map, the components', ``members``."""
    labelled = cfg["anomaly_labels"] is not None
    summary = [SUMMARY] + ([SUMMARY_LABELLED] if labelled else [])
    table = [(columns, "raw", cells) for columns, cells in summary]
    if _filtered(cfg):
        table += [(tuple("filtered_" + c for c in columns), "filtered", cells) for columns, cells in summary]
    if cfg["anomaly_min_component"] is not None:
        table += [(columns, "components", cells) for columns, cells in [COMPONENTS] + ([COMPONENTS_LABELLED] if labelled else [])]
    if _ensemble_specs(cfg) is not None:
        table.append((("members",), "raw", lambda s, j: [str(s["members"])]))
    return table


def score_header(table):
    return ["subject"] + [c for columns, _, _ in table for c in columns]


def score_row(table, name, summaries, j):
    """the cells of subject ``name``, number ``j`` of its batch; ``summaries``: {"raw" / "filtered" / "components": host summaries of the batch}"""
    row = {"subject": stem(name)}
    for columns, source, cells in table:
        row.update(zip(columns, cells(summaries[source], j), strict=True))
    return row


def _resolve_files(cfg):
    """host only, so the refusals come first: the subjects, per member the healing outputs of every subject, the label and the mask volumes (or None)"""
    files = list_inputs(cfg["validation_subjects"])
    specs = _ensemble_specs(cfg)      # K healings per subject, one fused map; None: the single healing of 7.11
    if specs is None:
        members = [find_healing_outputs(files, cfg["anomaly_codes"] or cfg["outputs_directory"], cfg["anomaly_weight"])]
    else:
        members = find_ensemble_outputs(files, specs, cfg["anomaly_weight"])
    label_files = match_labels(files, cfg["anomaly_labels"]) if cfg["anomaly_labels"] is not None else None
    mask_files = match_labels(files, cfg["anomaly_mask"], "anomaly_mask", "mask") if cfg["anomaly_mask"] not in (None, "scan") else None
    return files, members, label_files, mask_files


def _decode_members(net, cfg, members, picks, names, x):
    """per member the decoding [B, 1, D, H, W] of this batch's healed codes and the weight grids [B, d, h, w] (None with --anomaly_weight=none);
    member by member: each decode_samples call is the one a single-healing run makes for this batch"""
    recs, wgts = [], []
    for healed in members:
        grids, weights = [], []
        for n, p in zip(names, picks):
            h = healed[p]
            codes = np.load(h["healed"]).astype(np.int64)
            if codes.min() < 0 or codes.max() >= net.n_embed:      # the check of --mode=decoding
                raise ValueError(f"{h['healed']}: code {int(codes.max())} is not a codebook entry (num_embeddings={net.n_embed})")
            grids.append(torch.from_numpy(codes))
            if cfg["anomaly_weight"] != "none":
                wgt = np.load(h["resampled" if cfg["anomaly_weight"] == "mask" else "nll"]).astype(np.float32)
                if wgt.shape != codes.shape:
                    raise ValueError(f"{n}: the weight grid {wgt.shape} and the healed codes {codes.shape} differ in shape")
                weights.append(torch.from_numpy(wgt))
        recs.append(net.decode_samples([torch.stack(grids).to(x.device)]).float())
        if recs[-1].shape != x.shape:
            raise ValueError(f"{names[0]}: the healed codes decode to {tuple(recs[-1].shape[2:])}, the scan is {tuple(x.shape[2:])} (--roi?)")
        wgts.append(torch.stack(weights).to(x.device) if weights else None)
    return recs, wgts


def _map(cfg, x, recs, wgts, labels):
    kw = dict(sigma=_anomaly_sigma(cfg), residual=cfg["anomaly_residual"], labels=labels, threshold=cfg["anomaly_threshold"], hist_max=cfg["anomaly_hist_max"])
    if len(recs) == 1:
        return anomaly_map(x, recs[0], wgts[0], **kw)
    return anomaly_map_ensemble(x, torch.stack(recs), torch.stack(wgts) if wgts[0] is not None else None, **kw)      # one fused pass


def _filter(cfg, x, amap, masks, labels):
    """mask, median, mask again on the device; ``masks``: the batch's mask volumes, None with --anomaly_mask=scan or without a mask"""
    if cfg["anomaly_mask"] == "scan":
        masks = x > float(cfg["anomaly_mask_threshold"])
    return median_filter_map(amap, size=cfg["anomaly_median"] or 1, mask=masks, erosion=cfg["anomaly_mask_erosion"], labels=labels,
                             threshold=cfg["anomaly_threshold"], hist_max=cfg["anomaly_hist_max"])


def _components(cfg, amap, labels):
    """the cleaned segmentation {0, 1} of a map that is still on the device, and the components' summaries"""
    ids, summaries = connected_components(amap, threshold=cfg["anomaly_threshold"], connectivity=int(cfg["anomaly_connectivity"]),
                                          min_size=cfg["anomaly_min_component"], labels=labels)
    return (ids > 0).float(), summaries


def anomaly(cfg, rank, local, world, dev, build_network):
    """--mode=anomaly: every validation subject against the decoding of its healed codes, on the device from the scan to the scores."""
    import csv
    files, members, label_files, mask_files = _resolve_files(cfg)
    net = build_network(cfg, dev).eval()
    path = check_for_checkpoints(cfg)
    if path:
        load_network_state(net, path)
        log(rank, f"loaded {path}")
    gen = torch.Generator(device=dev).manual_seed(cfg["seed"] + rank)
    index = {f: k for k, f in enumerate(files)}
    order = shard_for_rank(len(files), rank, world, shuffle=False, pad=False)
    raw_cfg = dict(cfg, normalize=False)      # label and mask volumes: the scans' reorientation and ROI, never their normalisation

    def like_scans(volumes, picks, x):
        return torch.stack([_load_volume(volumes[p], raw_cfg, gen, dev).reshape(x.shape[1:]) for p in picks]) if volumes is not None else None
    posts = ["healed_reconstruction"] if len(members) == 1 else [f"healed_reconstruction_m{k}" for k in range(len(members))]
    writer, table, rows = VolumeWriter(cfg), score_table(cfg), []
    try:
        with torch.no_grad():
            for names, x, headers in _batches(files, order, cfg["eval_batch_size"], cfg, gen, dev):
                picks = [index[n] for n in names]
                recs, wgts = _decode_members(net, cfg, members, picks, names, x)
                labels = like_scans(label_files, picks, x)
                amap, raw = _map(cfg, x, recs, wgts, labels)
                outputs, summaries = {"anomaly_map": amap}, {"raw": raw}
                if _filtered(cfg):      # the components below take the filtered map
                    amap, summaries["filtered"] = _filter(cfg, x, amap, like_scans(mask_files, picks, x), labels)
                    outputs["anomaly_map_filtered"] = amap
                if cfg["anomaly_min_component"] is not None:
                    outputs["anomaly_segmentation"], summaries["components"] = _components(cfg, amap, labels)
                writer.batch()
                writer.save(names, {**outputs, **dict(zip(posts, recs))}, headers)
                host = {key: {k: v.cpu().numpy() if torch.is_tensor(v) else v for k, v in summ.items()} for key, summ in summaries.items()}
                rows += [score_row(table, n, host, j) for j, n in enumerate(names)]
    finally:
        writer.close()
    with open(os.path.join(cfg["outputs_directory"], f"anomaly_scores_rank{rank}.csv"), "w", newline="") as f:
        wr = csv.DictWriter(f, fieldnames=score_header(table))
        wr.writeheader()
        wr.writerows(rows)
    log(rank, f"anomaly done: {len(order)} subjects -> {cfg['outputs_directory']}")
