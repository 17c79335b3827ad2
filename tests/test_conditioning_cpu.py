"""CPU: conditioned training / sampling through the CLI, host side (reference run_transformer.py:81-95,160-215,340-373, src/utils/transformer.py:68-141,
225-235): the conditioning table loader with its refusals, the flags reaching ``run_transformer.build``, and the index rows that put both conditioning
types into the one embedding launch (src/networks/transformers/performer.py:252-266)."""
import warnings

import pytest
import torch

from synthanatomy_amd.utils.transformer import conditioning_batch, conditioning_flags, load_conditionings, prepare_batch

ROWS = [("subject", "age", "sex", "site"),
        ("s0_quantization_0.npy", "0", "1", "3"),
        ("s1_quantization_0.npy", "2.7", "0", "3"),
        ("s2_quantization_0.npy", "", "1", "3"),          # empty cell
        ("s3_quantization_0.npy", "1", "NaN", "3"),       # NaN cell
        ("s0_quantization_0.npy", "3", "0", "3"),         # a second row of s0: the first one wins
        ("elsewhere.npy", "4", "1", "9")]                 # matches no file, still counts for nunique
FILES = [f"/data/codes/s{i}_quantization_0.npy" for i in range(5)]      # s4 has no row


def _write(path, rows, sep):
    path.write_text("\n".join(sep.join(r) for r in rows) + "\n")
    return str(path)


@pytest.mark.parametrize("ext,sep", [(".csv", ","), (".tsv", "\t")])
def test_loader_matches_the_reference_rules(tmp_path, ext, sep):
    path = _write(tmp_path / ("cond" + ext), ROWS, sep)
    with pytest.warns(UserWarning) as rec:
        kept, values, num_tokens = load_conditionings(FILES, path, ("age", "sex"))
    # nunique over the WHOLE file, NaN / empty cells not counted: age {0, 2.7, 1, 3, 4}, sex {0, 1}
    assert num_tokens == [5, 2]
    # matched on the basename; s2 (empty age) and s3 (NaN sex) and s4 (no row) leave; the first row of s0 wins (age 0, not 3)
    assert kept == [FILES[0], FILES[1]]
    assert values == {"age": [0.0, 2.7], "sex": [1.0, 0.0]}
    msg = [str(w.message) for w in rec if "discarded" in str(w.message)]
    assert len(msg) == 1
    assert "3 were discarded during data loading" in msg[0]
    assert "1 did not have matching conditioning and 2 had conditioning that was NaN" in msg[0]
    # the float cell 2.7 reaches the network as 2 (.long() of prepare_batch, src/utils/transformer.py:275)
    batch = {"quantization": torch.zeros(2, 1, 2, 2, dtype=torch.long), **conditioning_batch(values, ("age", "sex"), [0, 1])}
    (_, cond), _ = prepare_batch(batch, torch.arange(4), 7, ("age", "sex"))
    assert [c.tolist() for c in cond] == [[[0], [2]], [[1], [0]]] and all(c.dtype == torch.int64 for c in cond)
    # one column, other subjects: nothing to warn about when every subject is covered
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        kept, values, num_tokens = load_conditionings(FILES[:2], path, ("sex",))
    assert (kept, values, num_tokens) == (FILES[:2], {"sex": [1.0, 0.0]}, [2])


def test_loader_refusals_name_the_flag_or_the_column(tmp_path):
    path = _write(tmp_path / "cond.csv", ROWS, ",")
    with pytest.raises(ValueError, match="Path is not a csv/tsv with file paths inside."):
        load_conditionings(FILES, str(tmp_path / "cond.txt"), ("age",))
    with pytest.raises(ValueError, match="Path is not a csv/tsv with file paths inside."):
        load_conditionings(FILES, str(tmp_path / "missing.csv"), ("age",))
    with pytest.raises(ValueError, match="column 'weight'"):
        load_conditionings(FILES, path, ("age", "weight"))
    nosub = _write(tmp_path / "nosub.csv", [("name", "age"), ("s0_quantization_0.npy", "0")], ",")
    with pytest.raises(ValueError, match="'subject' column"):
        load_conditionings(FILES, nosub, ("age",))
    # site has two distinct values over the file (3, 9): the value 3 is no index into 2 embedding rows
    with pytest.raises(ValueError) as exc:
        load_conditionings(FILES, path, ("site",))
    assert all(s in str(exc.value) for s in ("s0_quantization_0.npy", "'site'", "3.0"))
    neg = _write(tmp_path / "neg.csv", [("subject", "age"), ("s0_quantization_0.npy", "-2"), ("x", "0"), ("y", "1")], ",")
    with pytest.raises(ValueError, match="'age'"):
        load_conditionings(FILES, neg, ("age",))
    text = _write(tmp_path / "text.csv", [("subject", "sex"), ("s0_quantization_0.npy", "F")], ",")
    with pytest.raises(ValueError, match="'sex'"):
        load_conditionings(FILES, text, ("sex",))


def test_flag_combinations_act_or_refuse():
    assert conditioning_flags(None, None, "bos_replacement") is None and conditioning_flags(None, None, "none") is None
    assert conditioning_flags("c.csv", "age", "prepending") == ("age",)            # a single string is the 1-tuple
    assert conditioning_flags("c.csv", ["age", "sex"], "bos_replacement") == ("age", "sex")
    assert conditioning_flags("c.csv", "(age,sex)", "bos_replacement") == ("age", "sex")      # bare names on the command line, as python-fire reads them
    assert conditioning_flags("c.csv", "['age', 'sex']", "bos_replacement") == ("age", "sex")
    with pytest.raises(ValueError, match="--conditioning_path"):
        conditioning_flags(None, ("age",), "bos_replacement")
    with pytest.raises(ValueError, match="--conditionings"):
        conditioning_flags("c.csv", None, "bos_replacement")
    with pytest.raises(ValueError, match="--conditioning_type"):
        conditioning_flags("c.csv", ("age",), "appending")
    with pytest.raises(ValueError, match="--conditioning_type=none"):
        conditioning_flags("c.csv", ("age",), "none")


def test_cli_refuses_before_touching_the_gpu(tmp_path):
    import run_transformer
    base = ["--training_subjects=synthetic:1", "--validation_subjects=synthetic:1", f"--project_directory={tmp_path}/", "--experiment_name=e"]
    with pytest.raises(ValueError, match="--conditioning_path"):
        run_transformer.run(base + ["--conditionings=age"])
    with pytest.raises(ValueError, match="--conditionings"):
        run_transformer.run(base + [f"--conditioning_path={tmp_path}/c.csv"])
    with pytest.raises(ValueError, match="--conditioning_type"):
        run_transformer.run(base + ["--conditioning_type=appending"])


@pytest.mark.parametrize("ctype", ["bos_replacement", "prepending"])
def test_build_receives_the_conditioning_flags(tmp_path, ctype):
    import run_transformer
    path = _write(tmp_path / "cond.csv", ROWS, ",")
    cfg = dict(run_transformer.DEFAULTS, vocab_size=16, n_embd=32, n_layers=1, n_head=2, conditioning_path=path, conditioning_type=ctype,
               conditionings=conditioning_flags(path, ("age", "sex"), ctype))
    with pytest.warns(UserWarning):
        kept, values = run_transformer._conditioned_subjects(FILES, cfg, 0, "training")
    assert kept == FILES[:2] and cfg["conditioning_num_tokens"] == [5, 2]
    net, _ = run_transformer.build(cfg, (2, 3, 4), "cpu")
    assert [tuple(e.weight.shape) for e in net.conditioning_emb] == [(5, 32), (2, 32)] and net.conditioning_type == ctype
    assert net.max_seq_len == 25 + (2 if ctype == "prepending" else 0)
    assert {"conditioning_emb.0.weight", "conditioning_emb.1.weight"} <= set(net.state_dict())      # the reference's checkpoint keys
    plain, _ = run_transformer.build(dict(run_transformer.DEFAULTS, vocab_size=16, n_embd=32, n_layers=1, n_head=2), (2, 3, 4), "cpu")
    assert len(plain.conditioning_emb) == 0 and not any("conditioning_emb" in k for k in plain.state_dict()) and plain.max_seq_len == 25


def test_index_rows_of_both_conditioning_types():
    """B = 2, N = 5, c = 2: where the -1s sit, the reversed order for prepending, the shift of the spatial rows."""
    from synthanatomy_amd.networks.transformers.performer import conditioning_index_rows
    tok = torch.tensor([[9, 1, 2, 3, 4], [9, 5, 6, 7, 8]])
    sp = [torch.tensor([-1, 0, 0, 1, 1]), torch.tensor([-1, 0, 1, 0, 1])]
    conds = [torch.tensor([[3], [4]]), torch.tensor([6, 6])]          # [B, 1] as prepare_batch gives them, and plain [B]
    t, s, c, nt = conditioning_index_rows("bos_replacement", tok, sp, conds)
    assert nt == 5
    assert t.tolist() == [-1, 1, 2, 3, 4, -1, 5, 6, 7, 8]                       # position 0 loses its token
    assert [r.tolist() for r in s] == [r.tolist() for r in sp]                   # spatial rows: -1 at position 0 already
    assert c[0].tolist() == [3, -1, -1, -1, -1, 4, -1, -1, -1, -1]              # both tables land on position 0
    assert c[1].tolist() == [6, -1, -1, -1, -1, 6, -1, -1, -1, -1]
    assert tok.tolist()[0][0] == 9                                               # the caller's tokens are left alone
    t, s, c, nt = conditioning_index_rows("prepending", tok, sp, conds)
    assert nt == 7
    assert t.tolist() == [-1, -1, 9, 1, 2, 3, 4, -1, -1, 9, 5, 6, 7, 8]         # tokens move back by c
    assert [r.tolist() for r in s] == [[-1, -1, -1, 0, 0, 1, 1], [-1, -1, -1, 0, 1, 0, 1]]
    assert c[0].tolist() == [-1, 3, -1, -1, -1, -1, -1, -1, 4, -1, -1, -1, -1, -1]   # conditioning 0 at position c-1-0 = 1
    assert c[1].tolist() == [6, -1, -1, -1, -1, -1, -1, 6, -1, -1, -1, -1, -1, -1]   # the LAST conditioning comes first
    assert all(r.dtype == torch.int64 for r in [t] + s + c)
    with pytest.raises(ValueError):
        conditioning_index_rows("none", tok, sp, conds)
