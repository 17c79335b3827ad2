"""GPU: conditioned training and sampling (reference run_transformer.py:81-95,160-215,340-373, src/networks/transformers/performer.py:252-266,279-281).
Both conditioning types through the ONE embedding launch (sa_embed_sum / sa_embed_scatter / sa_embed_scatter_det with index rows that are -1 outside the
conditioning's position) against the CPU oracle restatement (oracle/performer_ref.py; parity UNPINNED against the third-party package -- see that file), the
O(N) sampler with prepended conditionings against the reference loop and the oracle's greedy chain, and the flags through run_transformer.py.

Tolerances: those of tests/test_performer_gpu.py::test_embedding_variants_match_oracle for the same quantities (logits 1e-3, gradients 3e-3, relative to
the largest reference magnitude)."""
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import performer_ref as P  # noqa: E402

REL, REL_GRAD = 1e-3, 3e-3
SHAPE, N, NCOND, DIM = (2, 3, 4), 24, (5, 7), 32


def _rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


def _net_and_state(ctype, ncond, num_tokens, seed, gate, extra=0, cond_scale=1.0):
    """the tiny network of the existing conditioning tests: grid (2, 3, 4), dim 32, depth 2, 4 heads of width 64 with 2 local, window 6; `extra` more
    positions for a given prefix longer than the BOS token; `cond_scale` scales the conditioning tables (prepended conditionings act through the
    attention layers only: at unit scale this network's greedy chain does not depend on them -- the oracle's does not either)"""
    from synthanatomy_amd.networks.transformers.img2seq_ordering import Ordering
    from synthanatomy_amd.networks.transformers.performer import Performer
    prep = ctype == "prepending"
    cfg = P.PerformerConfig(num_tokens=num_tokens, max_seq_len=N + extra + (len(ncond) if prep else 0), dim=DIM, depth=2, heads=4, dim_head=64,
                            local_attn_heads=2, local_window_size=6, spatial_shape=SHAPE)
    st = P.init_state(cfg, seed=seed, spatial_index_len=N - 1)
    g = torch.Generator().manual_seed(seed + 1)
    for i, c in enumerate(ncond):
        st[f"conditioning_emb.{i}.weight"] = cond_scale * torch.randn(c, DIM, generator=g)
    for k in st:
        if k.endswith(".g"):
            st[k] = torch.full_like(st[k], gate)
    o = Ordering("raster_scan", 3, (1,) + SHAPE, (False,) * 3, (), ())
    net = Performer(num_tokens=num_tokens, max_seq_len=N + extra, dim=DIM, depth=2, heads=4, ordering=o, dim_head=64, local_attn_heads=2,
                    local_window_size=6, use_rezero=True, spatial_position_emb="absolute", spatial_shape=SHAPE, feature_redraw_interval=None,
                    compute_dtype=torch.float32, conditioning_num_tokens=ncond, conditioning_type=ctype)
    missing, unexpected = net.load_state_dict({k: v.clone() for k, v in st.items()}, strict=False)
    assert not unexpected, unexpected
    assert all(("spatial_indices_sequence" in k or "inv_freq" in k or "calls_since" in k) for k in missing), missing
    return net.cuda(), st, cfg, o, P.spatial_index_sequences(SHAPE, o.get_sequence_ordering())


@pytest.mark.parametrize("ctype,n", [("bos_replacement", N), ("prepending", N), ("bos_replacement", 1)])
def test_conditioned_forward_and_gradients_through_the_single_launch(ctype, n, monkeypatch):
    """B = 3 with rows 0 and 2 sharing BOTH conditioning values (duplicate rows are what a scatter can get wrong); n = 1: the whole sequence is the replaced row."""
    from synthanatomy_amd import _ffi
    from synthanatomy_amd.losses.transformer import CELoss
    from synthanatomy_amd.networks.transformers import performer as perf
    net, st, cfg, o, seqs = _net_and_state(ctype, NCOND, 33, 11, 0.4)
    net.train()
    g = torch.Generator().manual_seed(3)
    tok = torch.randint(0, 33, (3, n), generator=g)
    tgt = torch.randint(0, 32, (3, n), generator=g)
    conds = [torch.tensor([[2], [4], [2]]), torch.tensor([[6], [0], [6]])]
    leaf = {k: v.clone().requires_grad_(True) for k, v in st.items() if "projection_matrix" not in k}
    stt = dict(st)
    stt.update(leaf)
    ref = P.forward(stt, cfg, tok, seqs, conds, ctype)
    P.ce_loss(ref, tgt).backward()
    # one embedding launch, and no torch.cat of the [B, N, dim] activation
    launches = []
    real_lib = _ffi.lib()

    class _Counting:
        def __getattr__(self, name):
            fn = getattr(real_lib, name)
            if name != "sa_embed_sum":
                return fn
            return lambda *a: (launches.append(name), fn(*a))[1]

    counting = _Counting()
    real_cat = torch.cat
    monkeypatch.setattr(perf._ffi, "lib", lambda: counting)
    monkeypatch.setattr(torch, "cat", lambda ts, *a, **k: (_ for _ in ()).throw(AssertionError("torch.cat of an activation"))
                        if any(t.dim() == 3 for t in ts) else real_cat(ts, *a, **k))
    out = net(tok.cuda(), conditionings=[c.cuda() for c in conds])
    monkeypatch.undo()
    assert launches == ["sa_embed_sum"]
    print(f"{ctype} n={n}: logits rel {_rel(out, ref):.2e}")
    assert out.shape == ref.shape == (3, n, 33) and _rel(out, ref) < REL
    CELoss()(out.transpose(1, 2), tgt.cuda()).backward()
    torch.cuda.synchronize()
    params = dict(net.named_parameters())
    checked = 0
    for k, p in leaf.items():
        if k not in params or p.grad is None:
            continue
        got = params[k].grad if params[k].grad is not None else torch.zeros_like(params[k])
        if float(p.grad.abs().max()) == 0:      # (n = 1, BOS replacement: the only token is replaced, token_emb and the spatial tables receive nothing)
            assert float(got.abs().max()) == 0.0, k
            continue
        print(f"  d {k}: rel {_rel(got, p.grad):.2e}")
        assert _rel(got, p.grad) < REL_GRAD, k
        checked += 1
    assert checked > 20
    for k in ("conditioning_emb.0.weight", "conditioning_emb.1.weight", "pos_emb.emb.weight") + (("token_emb.weight",) if n > 1 else ()):
        assert float(leaf[k].grad.abs().max()) > 0 and float(params[k].grad.abs().max()) > 0, k
    # rows the batch never named receive nothing
    assert float(params["conditioning_emb.0.weight"].grad[[0, 1, 3]].abs().max()) == 0.0


@pytest.mark.parametrize("ctype", ["bos_replacement", "prepending"])
def test_deterministic_conditioned_steps_are_bit_identical(ctype):
    """--deterministic: the conditioning tables' gradients come from sa_embed_scatter_det like every other embedding gradient"""
    from synthanatomy_amd import debug
    from synthanatomy_amd.losses.transformer import CELoss
    net, *_ = _net_and_state(ctype, NCOND, 33, 11, 0.4)
    net.train()
    g = torch.Generator().manual_seed(3)
    tok = torch.randint(0, 33, (4, N), generator=g).cuda()
    tgt = torch.randint(0, 32, (4, N), generator=g).cuda()
    conds = [torch.tensor([[2], [4], [2], [2]]).cuda(), torch.tensor([[6], [0], [6], [1]]).cuda()]
    was = debug.deterministic()
    debug.set_deterministic(True)
    try:
        runs = []
        for _ in range(2):
            for p in net.parameters():
                p.grad = None
            loss = CELoss()(net(tok, conditionings=conds).transpose(1, 2), tgt)
            loss.backward()
            torch.cuda.synchronize()
            runs.append((loss.detach().clone(), {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}))
    finally:
        debug.set_deterministic(was)
    (l0, g0), (l1, g1) = runs
    assert torch.equal(l0, l1)
    assert float(g0["conditioning_emb.0.weight"].abs().max()) > 0 and float(g0["conditioning_emb.1.weight"].abs().max()) > 0
    assert all(torch.equal(g0[k], g1[k]) for k in g0)


@pytest.mark.parametrize("c,plen", [(1, 1), (2, 1), (2, 3)])
def test_stateful_sampler_with_prepended_conditionings(c, plen):
    """O(N) decoding with `conditioning_type="prepending"` (performer.py:262-264 through transformer.py:58-101): token for token equal to the reference-faithful
    loop, with and without the captured graph, and (P = 1) to the CPU oracle's greedy chain.  A longer given prefix (P = 3) stays in place: the loop and the
    sampler continue it alike.  (The oracle, like the reference, cannot add spatial embeddings to a sequence longer than the grid, so the chain is P = 1.)"""
    ncond = NCOND[:c]
    net, st, cfg, o, seqs = _net_and_state("prepending", ncond, 19, 13, 0.7, extra=plen - 1, cond_scale=4.0)
    B = 3
    g = torch.Generator().manual_seed(5)
    given = torch.cat((torch.full((B, 1), 18, dtype=torch.long), torch.randint(0, 18, (B, plen - 1), generator=g)), 1)
    prefix = given.cuda()
    conds = [torch.randint(0, k, (B, 1), generator=g) for k in ncond]
    cd = [x.cuda() for x in conds]
    quad = net.sample(prefix, conditioning=cd, sample=False, stateful=False)
    fast = net.sample(prefix, conditioning=cd, sample=False, stateful=True)
    fast_eager = net.sample(prefix, conditioning=cd, sample=False, stateful=True, use_graph=False)
    assert quad.shape == (B, *SHAPE)
    assert torch.equal(fast, quad) and torch.equal(fast_eager, quad)
    conds2 = [(v + 1) % k for v, k in zip(conds, ncond)]
    other = net.sample(prefix, conditioning=[x.cuda() for x in conds2], sample=False, stateful=True)
    assert not torch.equal(other, fast)                                      # the conditioning matters
    if plen > 1:
        flipped = net.sample(torch.cat((prefix[:, :1], (prefix[:, 1:] + 1) % 18), 1), conditioning=cd, sample=False, stateful=True)
        assert not torch.equal(flipped, fast)                                # ... and so does the given prefix
        return

    def chain(cv):
        x = given.clone()
        for _ in range(N):
            x = torch.cat((x, P.forward(st, cfg, x, seqs, cv, "prepending")[:, -1].argmax(-1, keepdim=True)), 1)
        return x[:, 1:][:, o.get_revert_sequence_ordering()].reshape(B, *SHAPE)

    ref, ref2 = chain(conds), chain(conds2)
    assert all(not torch.equal(ref[b], ref2[b]) for b in range(B))          # other conditioning values: another sequence, for every sample
    assert torch.equal(fast.cpu(), ref) and torch.equal(other.cpu(), ref2)


KEPT = [i for i in range(42) if i not in (3, 41)]


def _name(i):
    return f"{'s' if i in KEPT else 'x'}{i:02d}_quantization_0.npy"


def _cli_project(tmp_path, bad_age=None):
    """42 tiny code grids and two conditioning files.  x03 has a NaN age and x41 no row at all; the glob `s*` names exactly the 40 subjects the files cover,
    in the same order, so a run without the flags over `s*` sees the batches of the conditioned run over all 42.  A kept subject's grid is ONE token
    repeated, a function of its (age, sex) row -- four combinations -- so that eighty steps teach the tiny network what only the conditioning can tell it:
    the oracle's restatement trained on the same schedule on the host reproduces each row's token from its conditioning with a logit margin above 2, for
    both types (with 20 subjects it does not yet, nor with six combinations).  Ages 0 and 1.7 (-> 1), and a 5 in a row that matches no file: three
    distinct values over the whole file.  `other.csv`: the same subjects and the same distinct values, every kept row the other age and the other sex."""
    codes = tmp_path / "codes"
    codes.mkdir()
    rows, other = ["subject,age,sex"], ["subject,age,sex"]
    cells = ("0", "1.7")
    for i in range(42):
        age, sex = i % 2, (i // 2) % 2
        np.save(codes / _name(i), np.full(SHAPE, 5 * age + 2 * sex, dtype=np.uint16))
        cell = "NaN" if i == 3 else bad_age if (bad_age and i == 2) else cells[age]
        if i != 41:
            rows.append(f"{_name(i)},{cell},{sex}")
            other.append(f"{_name(i)},{'NaN' if i == 3 else cells[1 - age]},{1 - sex}")
    (tmp_path / "cond.csv").write_text("\n".join(rows + ["elsewhere.npy,5,0"]) + "\n")
    (tmp_path / "other.csv").write_text("\n".join(other + ["elsewhere.npy,5,0"]) + "\n")
    common = ["--project_directory=" + str(tmp_path) + "/", "--vocab_size=16", "--n_embd=32", "--n_layers=2", "--n_head=4", "--local_attn_heads=2",
              "--local_window_size=6", "--use_rezero=False", "--spatial_position_emb=absolute", "--feature_redraw_interval=None", "--batch_size=1",
              "--eval_batch_size=10", "--log_every=1", "--learning_rate=1e-2"]
    every = ["--training_subjects=" + str(codes) + "/*_quantization_0.npy", "--validation_subjects=" + str(codes) + "/*_quantization_0.npy"]
    covered = ["--training_subjects=" + str(codes) + "/s*_quantization_0.npy", "--validation_subjects=" + str(codes) + "/s*_quantization_0.npy"]
    return common, every, covered, ["--conditionings=(age,sex)"]


def _losses(text):
    return [float(l.split(" loss ")[1].split()[0]) for l in text.splitlines() if " loss " in l]


@pytest.mark.parametrize("ctype", ["bos_replacement", "prepending"])
def test_cli_trains_and_samples_conditioned(tmp_path, capsys, ctype):
    import run_transformer
    common, every, covered, cond = _cli_project(tmp_path)
    cond = cond + ["--conditioning_type=" + ctype]
    path, other = ["--conditioning_path=" + str(tmp_path / "cond.csv")], ["--conditioning_path=" + str(tmp_path / "other.csv")]
    train = ["--mode=training", "--epochs=2", "--checkpoint_every=1", "--eval_every=2"]
    with pytest.warns(UserWarning, match="1 did not have matching conditioning and 1 had conditioning that was NaN"):
        run_transformer.run(common + every + cond + path + train + ["--experiment_name=cond"])
    log = capsys.readouterr().out
    assert "The conditioning vocab size is modified as follows:" in log and "To [3, 2] due to sex." in log      # ages {0, 1.7, 5} over the WHOLE file
    assert "training subjects with conditioning ('age', 'sex'): 40 of 42" in log
    assert len(_losses(log)) == 80 and "validation ce" in log                # 40 kept subjects, batch 1, 2 epochs
    ck = glob.glob(str(tmp_path) + "/cond/performer/checkpoints/checkpoint_epoch=2.pt")
    assert ck
    sd = torch.load(ck[0], map_location="cpu", weights_only=False)["network"]
    assert sd["conditioning_emb.0.weight"].shape == (3, 32) and sd["conditioning_emb.1.weight"].shape == (2, 32)
    torch.manual_seed(2)                                                      # run() seeds with --seed=2 before it builds the network
    np.random.seed(2)
    init, _ = run_transformer.build(dict(run_transformer.DEFAULTS, vocab_size=16, n_embd=32, n_layers=2, n_head=4, local_attn_heads=2, local_window_size=6,
                                         use_rezero=False, spatial_position_emb="absolute", feature_redraw_interval=None, conditionings=("age", "sex"),
                                         conditioning_num_tokens=[3, 2], conditioning_type=ctype), SHAPE, "cpu")
    used = [0, 1]                                                             # the ages of the kept subjects, truncated
    assert torch.equal(init.conditioning_emb[0].weight[2], sd["conditioning_emb.0.weight"][2])           # same initial values: the unused row stays
    assert float((init.conditioning_emb[0].weight.detach()[used] - sd["conditioning_emb.0.weight"][used]).abs().max(1).values.min()) > 0    # the used rows moved
    # the same run without the flags over the 40 covered subjects: the same batches in the same order, another loss
    run_transformer.run(common + covered + train + ["--experiment_name=plain"])
    plain = capsys.readouterr().out
    assert "conditioning" not in plain and len(_losses(plain)) == 80
    assert _losses(plain)[0] != _losses(log)[0]
    # ... and the same conditioned run on other VALUES: the same network at the first step (seed, table sizes), the same subject in the batch -- only
    # what the conditioning rows say differs, so the first loss differs only if the values reach the network
    run_transformer.run(common + covered + cond + other + ["--mode=training", "--epochs=1", "--checkpoint_every=1", "--experiment_name=other"])
    log2 = capsys.readouterr().out
    assert "To [3, 2] due to sex." in log2 and "training subjects with conditioning ('age', 'sex'): 40 of 40" in log2
    assert _losses(log2)[0] != _losses(log)[0]
    # inference: one sample per kept validation subject, each conditioned on its own row
    with pytest.warns(UserWarning, match="were discarded"):
        run_transformer.run(common + every + cond + path + ["--mode=inference", "--sample=False", "--experiment_name=cond"])
    out = sorted(glob.glob(str(tmp_path) + "/cond/performer/outputs/*/*_sample.npy"))
    assert [os.path.basename(f) for f in out] == [f"s{i:02d}_quantization_0_sample.npy" for i in KEPT]
    smp = {int(os.path.basename(f)[1:3]): np.load(f) for f in out}
    assert all(v.shape == SHAPE and v.dtype == np.uint16 and v.max() < 16 for v in smp.values())
    # inference reads no codes: the subjects differ in nothing but their conditioning rows.  Equal rows -> equal greedy samples; s00 (age 0, sex 0)
    # against s01 (age 1, sex 0) and against s02 (age 0, sex 1): another age, or another sex, another sample
    assert np.array_equal(smp[0], smp[4]) and np.array_equal(smp[1], smp[5])
    assert not np.array_equal(smp[0], smp[1]) and not np.array_equal(smp[0], smp[2])


def test_cli_stops_on_an_out_of_range_value_before_any_kernel_runs(tmp_path, monkeypatch):
    import run_transformer
    from synthanatomy_amd import _ffi
    common, every, covered, cond = _cli_project(tmp_path, bad_age="7")        # ages 0, 1.7, 7 and the 5 of the unmatched row: 7 is no index into 4 rows
    monkeypatch.setattr(_ffi, "lib", lambda: (_ for _ in ()).throw(AssertionError("a kernel library call before the refusal")))
    with pytest.raises(ValueError) as exc:
        run_transformer.run(common + every + cond + ["--conditioning_path=" + str(tmp_path / "cond.csv"), "--mode=training", "--epochs=1",
                                                     "--experiment_name=bad", "--conditioning_type=prepending"])
    assert all(s in str(exc.value) for s in ("s02_quantization_0.npy", "'age'", "7.0"))
    assert not glob.glob(str(tmp_path) + "/bad/performer/checkpoints/*.pt")
