"""GPU, world_size 2 on ONE MI355X (gloo over device tensors, as tests/test_ddp_gpu.py): dead-code restarts on the data-parallel path -- the donor rows travel
in the packed statistics all-reduce, the decision is read from the all-reduced counts -- against ONE process on the concatenated batch.  The restarted ids, the
idle counters, ``info`` and the restarted rows of ``N`` / ``embed_avg`` are the same bits everywhere; the rest agrees to tests/test_ddp_gpu.py's tolerance (the
sum over ranks rounds differently from the sum over one long batch)."""
import os
import socket
import tempfile

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

K, D, P, R, SEED, STEPS, DECAY = 16, 8, 2, 4, 4, 4, 0.75


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _steps(rank, world):
    """STEPS training forwards of one quantizer on this rank's half (world 2) or on the whole (world 1) of a seeded batch of 2 x 64 rows"""
    from synthanatomy_amd import debug
    from synthanatomy_amd.networks.vqvae.baseline import Quantizer
    debug.set_deterministic(True)
    torch.manual_seed(2)
    q = Quantizer(n_embed=K, embed_dim=D, decay=DECAY)
    w0 = q.impl.weight.detach().clone()
    q = q.cuda().train()
    q.impl.set_restart(P, R, SEED)
    out = []
    for step in range(STEPS):
        g = torch.Generator().manual_seed(100 + step)
        which = torch.where(torch.rand(128, generator=g) < 0.5, 3, 9)
        rows = w0[which] + 0.01 * torch.randn(128, D, generator=g)
        x = rows.reshape(2, 4, 4, 4, D).permute(0, 4, 1, 2, 3).contiguous()
        per = 2 // world
        q.impl._restart_step = step
        q(x[rank * per:(rank + 1) * per].cuda())
        info = q.impl.restart_info()
        torch.cuda.synchronize()
        out.append(dict(info=info, idle=q.impl.idle.cpu().clone(), N=q.impl.N.cpu().clone(), embed_avg=q.impl.embed_avg.cpu().clone(),
                        weight=q.impl.weight.detach().cpu().clone()))
    debug.set_deterministic(False)
    return out


def _worker(rank, world, port, outdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")   # both ranks on cuda:0
    import torch.distributed as dist

    from synthanatomy_amd.runtime.ddp import init_distributed
    r, _l, w = init_distributed(backend="gloo")
    assert (r, w) == (rank, world)
    torch.save(_steps(rank, world), os.path.join(outdir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def _close(a, b, rtol=1e-5):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30)) <= rtol


def test_two_ranks_restart_the_same_codes_from_the_same_rows():
    full = _steps(0, 1)
    with tempfile.TemporaryDirectory() as d:
        ctx = mp.get_context("spawn")
        port = _free_port()
        procs = [ctx.Process(target=_worker, args=(r, 2, port, d)) for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(timeout=300)
            assert p.exitcode == 0, p.exitcode
        ranks = [torch.load(os.path.join(d, f"rank{r}.pt"), weights_only=False) for r in range(2)]
    assert [s["info"]["restarted"] for s in full] == [0, 4, 4, 4] and full[1]["info"]["ids"] == [0, 1, 2, 4]
    for step in range(STEPS):
        f = full[step]
        ids = f["info"]["ids"]
        for r in ranks:
            s = r[step]
            assert s["info"] == f["info"], (step, s["info"], f["info"])
            assert torch.equal(s["idle"], f["idle"]), step
            assert torch.equal(s["N"][ids], f["N"][ids]) and torch.equal(s["embed_avg"][ids], f["embed_avg"][ids]), step      # (1 - decay) . donor, exactly
            for k in ("N", "embed_avg", "weight"):
                assert _close(s[k], f[k]), (step, k)
        for k in ("idle", "N", "embed_avg", "weight"):      # the two ranks hold bit-identical replicas
            assert torch.equal(ranks[0][step][k], ranks[1][step][k]), (step, k)
    # the donors came from BOTH ranks' rows at some step: row g of the global batch is local row g mod 64 of rank g // 64
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import vq_restart_ref as ref
    owners = {g // 64 for step in range(STEPS) for g in ref.donor_indices(128, R, SEED, step)}
    assert owners == {0, 1}
