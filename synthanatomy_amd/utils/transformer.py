"""Batch preparation for the transformer stage -- mirror of reference src/utils/transformer.py:239-317.

``prepare_batch``: flatten the code grid, re-order it with the ordering's index sequence, left-pad the begin-of-sequence
token (== ``vocab_size``), and split into (input, target) shifted by one.  ``prepare_inference_batch``: ``[B, 1]`` of BOS.
Integer host/device glue; bit-exact with the reference by construction (pinned in tests/test_host_logic.py).

``conditioning_flags`` / ``load_conditionings``: the conditioning table of ``get_subjects`` (src/utils/transformer.py:68-141) on the stdlib ``csv``
module, with the refusals the reference lacks.
"""
from __future__ import annotations

import csv
import math
import os
import warnings
from enum import Enum

import numpy as np
import torch
import torch.nn.functional as F


class TransformerConditioningType(Enum):
    NONE = "none"
    BOSREPLACEMENT = "bos_replacement"
    PREPENDING = "prepending"


_NA_CELLS = frozenset(("", "#N/A", "#N/A N/A", "#NA", "-1.#IND", "-1.#QNAN", "-NaN", "-nan", "1.#IND", "1.#QNAN", "<NA>", "N/A", "NA", "NULL", "NaN", "None",
                       "n/a", "nan", "null"))   # what pandas.read_csv reads as NaN by default


def conditioning_flags(conditioning_path, conditionings, conditioning_type):
    """``--conditioning_path`` / ``--conditionings`` / ``--conditioning_type`` checked as a set -> the tuple of column names, or None without conditioning.
    A single string means the 1-tuple; ``"(age,sex)"`` with bare names is read as python-fire reads it.  Every inconsistent combination is a ``ValueError`` that names the flag: the flags act or refuse."""
    choices = [t.value for t in TransformerConditioningType]
    if conditioning_type not in choices:
        raise ValueError(f"--conditioning_type unknown. Was given {conditioning_type!r} but choices are {choices}.")
    if isinstance(conditionings, str):       # `--conditionings=age`, or `--conditionings=(age,sex)` with bare names (python-fire reads that as a tuple of strings)
        conditionings = tuple(c.strip(" '\"") for c in conditionings.strip().strip("()[]").split(",") if c.strip(" '\""))
    conditionings = tuple(conditionings) if conditionings else None
    if conditionings and not all(isinstance(c, str) and c for c in conditionings):
        raise ValueError(f"--conditionings must name columns of the conditioning file, got {conditionings!r}")
    if conditionings and not conditioning_path:
        raise ValueError(f"--conditionings={conditionings!r} needs --conditioning_path (the csv/tsv that holds those columns)")
    if conditioning_path and not conditionings:
        raise ValueError(f"--conditioning_path={conditioning_path!r} needs --conditionings (the columns to condition on)")
    if conditionings and conditioning_type == TransformerConditioningType.NONE.value:
        raise ValueError(f"--conditionings={conditionings!r} with --conditioning_type=none would be ignored; choose 'bos_replacement' or 'prepending'")
    return conditionings


def _cell(text, column):
    """one csv cell as pandas would read a numeric column: a float, NaN for the empty / NA spellings"""
    text = (text or "").strip()
    if text in _NA_CELLS:
        return math.nan
    try:
        return float(text)
    except ValueError:
        raise ValueError(f"conditioning column '{column}' holds the non-numeric value {text!r}") from None


def load_conditionings(subject_files, conditioning_path, conditionings):
    """``get_subjects`` (src/utils/transformer.py:68-141) without pandas.

    ``conditioning_path``: a ``.csv`` (comma) or ``.tsv`` (tab) with a ``subject`` column and one numeric column per name in ``conditionings``.  A subject
    file is matched on ``os.path.basename(file) == subject`` (first matching row wins); one without a row, or with a NaN / empty cell in a requested
    column, is discarded -- one warning carries the reference's wording and both counts.  ``conditioning_num_tokens[i]`` is the number of distinct non-NaN
    values of column i over the WHOLE file (pandas ``nunique``, :104), so training and inference on the same file build the same tables.

    Returns ``(kept_files, values, conditioning_num_tokens)``; ``values[name][k]`` is the float cell of kept subject k (``prepare_batch`` truncates it
    with ``.long()``, :275).  Beyond the reference: a missing ``subject`` / requested column and a value whose truncation lies outside
    ``[0, conditioning_num_tokens[i])`` are ``ValueError``s -- upstream would index past the end of the embedding table on the device."""
    conditionings = tuple(conditionings)
    if not (isinstance(conditioning_path, str) and os.path.isfile(conditioning_path) and conditioning_path.endswith((".csv", ".tsv"))):
        raise ValueError("Path is not a csv/tsv with file paths inside.")
    with open(conditioning_path, newline="") as f:
        reader = csv.DictReader(f, delimiter="\t" if conditioning_path.endswith(".tsv") else ",")
        header = [h.strip() for h in (reader.fieldnames or [])]
        reader.fieldnames = header
        rows = list(reader)
    if "subject" not in header:
        raise ValueError(f"--conditioning_path={conditioning_path!r} has no 'subject' column (columns: {header})")
    for c in conditionings:
        if c not in header:
            raise ValueError(f"--conditionings: column '{c}' is not in {conditioning_path!r} (columns: {header})")
    table = {c: [_cell(r.get(c), c) for r in rows] for c in conditionings}
    num_tokens = [len({v for v in table[c] if not math.isnan(v)}) for c in conditionings]
    first_row = {}
    for k, r in enumerate(rows):
        first_row.setdefault((r.get("subject") or "").strip(), k)
    kept, values = [], {c: [] for c in conditionings}
    mia_subjects = nan_subjects = 0
    for file in subject_files:
        name = os.path.basename(file)
        k = first_row.get(name)
        if k is None:
            mia_subjects += 1
            continue
        row = [table[c][k] for c in conditionings]
        if any(math.isnan(v) for v in row):
            nan_subjects += 1
            continue
        for c, v, n in zip(conditionings, row, num_tokens):
            if math.isinf(v) or not 0 <= int(v) < n:     # int() truncates towards zero, as .long() does
                raise ValueError(f"subject '{name}': conditioning column '{c}' holds {v!r}, whose integer part is not an index into the {n} embedding rows "
                                 f"(the number of distinct values of '{c}' in {conditioning_path!r}); recode the column to 0 .. {n - 1}")
        kept.append(file)
        for c, v in zip(conditionings, row):
            values[c].append(v)
    if mia_subjects > 0 or nan_subjects > 0:
        warnings.warn(f"{mia_subjects + nan_subjects} were discarded during data loading. {mia_subjects} did not have matching conditioning and "
                      f"{nan_subjects} had conditioning that was NaN. Make sure your conditioning data covers all of your subjects.")
    return kept, values, num_tokens


def conditioning_batch(values, conditionings, picks):
    """the conditioning entries of one batch dict: ``{name: float64 tensor [len(picks)]}`` of the kept subjects ``picks``"""
    return {c: torch.tensor([values[c][k] for k in picks], dtype=torch.float64) for c in (conditionings or ())}


def _to(t, device, non_blocking):
    return t.to(device=device, non_blocking=non_blocking) if device is not None else t


def _conditionings(batch, conditionings, device, non_blocking):
    if not conditionings:
        return None
    out = []
    for label in conditionings:
        c = batch[label]
        if len(c.shape) == 1:
            c = c[..., None]
        out.append(_to(c.long(), device, non_blocking))
    return out


def prepare_batch(batch, index_sequence, vocab_size, conditionings=None, device=None, non_blocking=False):
    encoded = batch["quantization"]
    encoded = encoded.reshape(encoded.shape[0], -1)
    encoded = encoded[:, index_sequence]
    encoded = F.pad(encoded, (1, 0), "constant", vocab_size)
    encoded = encoded.long()
    conditioned = _conditionings(batch, conditionings, device, non_blocking)
    x_input = _to(encoded[:, :-1], device, non_blocking)
    x_target = _to(encoded[:, 1:], device, non_blocking)
    return (x_input, conditioned), x_target


def prepare_inference_batch(batch, num_embeddings, conditionings=None, device=None, non_blocking=False):
    no_samples = batch["quantization"].shape[0]
    initial = torch.from_numpy(np.repeat(np.array([[num_embeddings]]), no_samples, axis=0)).long()
    conditioned = _conditionings(batch, conditionings, device, non_blocking)
    return (_to(initial, device, non_blocking), conditioned), _to(initial, device, non_blocking)
