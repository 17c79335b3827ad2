"""GPU: BaselineVQVAE with sampling geometries beyond (4,2,1,1) / (4,2,1,0,1) -- odd extents with output_padding, kernels 2 and 3, a dilated stride-1
level -- against the CPU oracle (oracle/vqvae_ref.py passes stride, padding, output_padding and dilation to torch): encoder output, code indices,
decoder output and one training step's parameter gradients, plus one pass of configuration A through the run_vqvae.py CLI."""
import glob

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

torch.set_num_threads(min(16, torch.get_num_threads()))

# name -> (downsample, upsample, input extents, latent extents, seed)
CONFIGS = {
    "A": (((4, 2, 1, 1),) * 3, ((4, 2, 1, 1, 1), (4, 2, 1, 0, 1), (4, 2, 1, 1, 1)), (37, 45, 53), (4, 5, 6), 20),
    "B": (((3, 2, 1, 1), (2, 2, 0, 1)), ((2, 2, 0, 0, 1), (3, 2, 1, 1, 1)), (24, 20, 28), (6, 5, 7), 23),
    "C": (((4, 2, 1, 1), (3, 1, 2, 2)), ((3, 1, 2, 0, 2), (4, 2, 1, 0, 1)), (16, 12, 20), (8, 6, 10), 21),
}
BATCH = 2


def _relerr(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.abs(got - ref).max() / (np.abs(ref).max() + 1e-30)


_ORACLE = {}


def _oracle(name):
    """cfg, state, input and the oracle's fp32 / rounded results of one configuration, computed once and shared (read-only)"""
    if name in _ORACLE:
        return _ORACLE[name]
    from oracle import vqvae_ref
    down, up, dims, latent, seed = CONFIGS[name]
    cfg = vqvae_ref.VQVAEConfig(n_levels=len(down), downsample_parameters=down, upsample_parameters=up, n_embed=64, embed_dim=16, n_channels=32,
                                n_res_channels=32, n_res_layers=1)
    st = vqvae_ref.init_state(cfg, seed=seed)
    torch.manual_seed(seed + 100)
    x = torch.rand(BATCH, 1, *dims)
    gen = torch.Generator().manual_seed(seed + 200)
    rand_idx = torch.randint(0, 64, (BATCH, *latent), generator=gen)
    res = dict(cfg=cfg, st=st, x=x, rand_idx=rand_idx)
    with torch.no_grad():
        # precondition of the index comparison: in fp64 the best code of every latent voxel leads the second best by >= 1e-2 relative, so rounding cannot flip it
        st64 = {k: v.double() for k, v in st.items()}
        z64 = vqvae_ref.encode(st64, cfg, x.double())
        flat = z64.permute(0, 2, 3, 4, 1).reshape(-1, 16)
        W = st64["quantizer.0.impl.weight"]
        d2 = ((flat[:, None, :] - W[None]) ** 2).sum(-1)
        two = torch.topk(d2, 2, dim=1, largest=False).values
        res["gap"] = float(((two[:, 1] - two[:, 0]) / two[:, 1]).min())
        res["idx64"] = d2.argmin(dim=1).view(BATCH, *z64.shape[2:])
        for mode, rd, erd in (("f32", None, None), ("bf16", torch.bfloat16, torch.float16)):
            ref = vqvae_ref.forward({k: v.clone() for k, v in st.items()}, cfg, x, training=False, round_dtype=rd, enc_round_dtype=erd)
            res[mode] = dict(z=ref["z"], idx=ref["indices"], rec=vqvae_ref.decode(st, cfg, vqvae_ref.embed(st, rand_idx), round_dtype=rd))
    _ORACLE[name] = res
    return res


def _net(name, dtype):
    from synthanatomy_amd.networks.vqvae.baseline import BaselineVQVAE
    o = _oracle(name)
    cfg = o["cfg"]
    net = BaselineVQVAE(n_levels=cfg.n_levels, downsample_parameters=cfg.downsample_parameters, upsample_parameters=cfg.upsample_parameters, n_embed=64,
                        embed_dim=16, n_channels=32, n_res_channels=32, n_res_layers=1, compute_dtype=dtype)
    net.load_state_dict({k: v.clone() for k, v in o["st"].items()})
    return net.cuda()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_eval_paths_match_oracle(name, dtype):
    o = _oracle(name)
    dims, latent = CONFIGS[name][2], CONFIGS[name][3]
    ref = o["f32" if dtype == torch.float32 else "bf16"]
    net = _net(name, dtype).eval()
    x = o["x"].cuda()
    with torch.no_grad():
        z = net.encode(x)[0]
        idx = net.index_quantize(x)[0]
        rec = net.decode_samples([o["rand_idx"].cuda()])
        full = net(x)["reconstruction"][0]
    tol = 1e-3 if dtype == torch.float32 else 2e-2
    assert tuple(z.shape) == (BATCH, 16, *latent) and tuple(rec.shape) == (BATCH, 1, *dims) and tuple(full.shape) == (BATCH, 1, *dims)
    ez, er = _relerr(z.cpu().numpy(), ref["z"].numpy()), _relerr(rec.float().cpu().numpy(), ref["rec"].numpy())
    print(f"[{name} {dtype}] z rel err {ez:.2e}, decode_samples rel err {er:.2e}, fp64 code gap {o['gap']:.3f}")
    assert ez < tol, ez
    assert er < tol, er
    assert o["gap"] >= 1e-2, o["gap"]          # precondition: no index can flip within the tolerance
    assert torch.equal(idx.cpu(), o["idx64"]), float((idx.cpu() != o["idx64"]).float().mean())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_training_step_gradients_match_oracle(name, dtype):
    from oracle import vqvae_ref
    o = _oracle(name)
    cfg, st, x = o["cfg"], o["st"], o["x"]
    leaf = {k: v.clone().requires_grad_(True) for k, v in st.items() if "quantizer" not in k}
    stt = {k: v.clone() for k, v in st.items()}
    stt.update(leaf)
    rd, erd = (None, None) if dtype == torch.float32 else (torch.bfloat16, torch.float16)
    ref = vqvae_ref.forward(stt, cfg, x, training=True, round_dtype=rd, enc_round_dtype=erd)
    vqvae_ref.mse_loss(ref, x).backward()
    net = _net(name, dtype).train()
    out = net(x.cuda())
    loss = torch.nn.functional.mse_loss(out["reconstruction"][0].float(), x.cuda()) + out["quantization_losses"][0]
    loss.backward()
    torch.cuda.synchronize()
    params = dict(net.named_parameters())
    worst, where = 0.0, None
    for k, p in leaf.items():
        gr = params[k].grad
        assert gr is not None and torch.isfinite(gr).all(), k
        e = _relerr(gr.cpu().numpy(), p.grad.numpy())
        if e > worst:
            worst, where = e, k
    print(f"[{name} {dtype}] worst gradient rel err {worst:.2e} at {where}")
    assert worst < (2e-3 if dtype == torch.float32 else 8e-2), (worst, where)


def test_cli_configuration_a(tmp_path):
    """two training epochs on four synthetic 37 x 45 x 53 volumes, then extracting and decoding: every stage at odd extents through run_vqvae.py"""
    import run_vqvae
    proj = str(tmp_path) + "/"
    down, up = CONFIGS["A"][0], CONFIGS["A"][1]
    fmt = lambda t: "(" + ",".join("(" + ",".join(map(str, u)) + ")" for u in t) + ")"
    vq = ["--project_directory=" + proj, "--experiment_name=geo", "--no_levels=3", "--downsample_parameters=" + fmt(down), "--upsample_parameters=" + fmt(up),
          "--no_channels=32", "--num_embeddings=(64,)", "--embedding_dim=(16,)", "--decay=(0.5,)", "--roi=((0,37),(0,45),(0,53))", "--batch_size=2",
          "--eval_batch_size=2", "--loss=mse", "--learning_rate=1e-3"]
    run_vqvae.run(vq + ["--training_subjects=synthetic:4", "--validation_subjects=synthetic:2", "--mode=training", "--epochs=2"])
    assert len(glob.glob(proj + "geo/baseline_vqvae/checkpoints/checkpoint_epoch=*.pt")) == 1
    run_vqvae.run(vq + ["--training_subjects=synthetic:4", "--validation_subjects=synthetic:2", "--mode=extracting"])
    codes = sorted(glob.glob(proj + "geo/baseline_vqvae/outputs/*/*_quantization_0.npy"))
    assert len(codes) == 2
    c0 = np.load(codes[0])
    assert c0.dtype == np.uint16 and c0.shape == (4, 5, 6) and c0.max() < 64
    rec = np.load(codes[0].replace("quantization_0", "reconstruction"))
    assert rec.shape == (37, 45, 53) and np.isfinite(rec).all()
    run_vqvae.run(vq + ["--training_subjects=" + proj + "geo/baseline_vqvae/outputs/*/*_quantization_0.npy", "--validation_subjects=synthetic:1", "--mode=decoding"])
    dec = glob.glob(proj + "geo/baseline_vqvae/outputs/*/*_sample.npy")
    assert len(dec) == 2 and np.load(dec[0]).shape == (37, 45, 53)
