"""Dead-code restarts of the EMA quantizer on the GPU: ``sa_vq_restart_donors`` against its numpy restatement, ``sa_vq_ema_update_restart``
against the identity that defines it (bit for bit ``sa_vq_ema_update`` on substituted inputs; idle counters and ``info`` against tests/vq_restart_ref.py),
the quantizer module's step sequence, and resuming through the ``codebook_restart`` state object."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vq_restart_ref as ref  # noqa: E402

DECAY, EPS = 0.75, 1e-5
INT32_MAX = ref.INT32_MAX


def _lib():
    from synthanatomy_amd import _ffi
    return _ffi, _ffi.lib(), _ffi.stream()


def _gather(rows, R, seed, step, row_base=0, Mtot=None):
    _ffi, lib, st = _lib()
    M, D = rows.shape
    d = torch.from_numpy(rows).cuda()
    out = torch.full((R, D), 7.0, device="cuda")      # every slot must be written
    _ffi.check(lib.sa_vq_restart_donors(_ffi.ptr(d), M, D, row_base, M if Mtot is None else Mtot, R, seed, step, _ffi.ptr(out), st), "sa_vq_restart_donors")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ donors
@pytest.mark.parametrize("M,D,R", [(37, 8, 4), (3, 8, 8), (64, 256, 32)])
def test_donors_match_the_restatement(M, D, R):
    rows = np.random.default_rng(M).standard_normal((M, D)).astype(np.float32)
    for seed, step in ((4, 0), (4, 5), ((9 << 32) + 1, (3 << 32) + 7)):
        got = _gather(rows, R, seed, step)
        want = ref.donors(rows, R, seed, step)
        assert np.array_equal(_bits(got), _bits(want)), (seed, step)
        if R > M:
            assert not got[M:].any()      # slots beyond R_eff = min(R, Mtot) are zero


def test_donor_buffers_of_two_ranks_sum_to_the_single_gather():
    rows = np.random.default_rng(1).standard_normal((74, 8)).astype(np.float32)
    whole = _gather(rows, 4, 11, 3)
    a = _gather(rows[:37], 4, 11, 3, row_base=0, Mtot=74)
    b = _gather(rows[37:], 4, 11, 3, row_base=37, Mtot=74)
    assert np.array_equal(_bits(a), _bits(ref.donors(rows[:37], 4, 11, 3, 0, 74))) and np.array_equal(_bits(b), _bits(ref.donors(rows[37:], 4, 11, 3, 37, 74)))
    assert a.any() and b.any()      # (seed 11, step 3 puts donors on both halves)
    assert np.array_equal(_bits(a + b), _bits(whole))
    assert np.array_equal(_bits(whole), _bits(rows[ref.donor_indices(74, 4, 11, 3)]))


# ------------------------------------------------------------------------------------------------ the update
def _ema(N, avg, counts, dw, K, D):
    """sa_vq_ema_update on host arrays -> (N, embed_avg, codebook)"""
    _ffi, lib, st = _lib()
    t = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda() for a in (N, avg, counts, dw)]
    cb = torch.zeros(K, D, device="cuda")
    _ffi.check(lib.sa_vq_ema_update(_ffi.ptr(t[0]), _ffi.ptr(t[1]), _ffi.ptr(cb), _ffi.ptr(t[2]), _ffi.ptr(t[3]), K, D, DECAY, EPS, st), "sa_vq_ema_update")
    torch.cuda.synchronize()
    return t[0].cpu().numpy(), t[1].cpu().numpy(), cb.cpu().numpy()


class _Device:
    """the state of one quantizer on the device, statistics in ONE packed buffer [counts | dw | donors] as the module keeps them (K no multiple of 4: the
    dw and donor parts are not 16-byte aligned)"""

    def __init__(self, N, avg, idle, K, D, R):
        self.K, self.D, self.R = K, D, R
        self.N, self.avg = torch.from_numpy(N.copy()).cuda(), torch.from_numpy(avg.copy()).cuda()
        self.cb = torch.zeros(K, D, device="cuda")
        self.idle = torch.from_numpy(idle.copy()).cuda()
        self.stats = torch.zeros(K + K * D + R * D, device="cuda")
        self.info = torch.full((2 + R,), -9, dtype=torch.int32, device="cuda")

    def update(self, counts, dw, donor_rows, patience):
        _ffi, lib, st = _lib()
        K, D, R = self.K, self.D, self.R
        self.stats.copy_(torch.from_numpy(np.concatenate([counts.ravel(), dw.ravel(), donor_rows.ravel()])))
        c, w, d = self.stats[:K], self.stats[K:K + K * D], self.stats[K + K * D:]
        _ffi.check(lib.sa_vq_ema_update_restart(_ffi.ptr(self.N), _ffi.ptr(self.avg), _ffi.ptr(self.cb), _ffi.ptr(c), _ffi.ptr(w), K, D, DECAY, EPS,
                                                _ffi.ptr(self.idle), patience, _ffi.ptr(d), R, _ffi.ptr(self.info), st), "sa_vq_ema_update_restart")
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in (self.N, self.avg, self.cb, self.idle, self.info)]


def _case(K, D, kind, R, P, rng):
    """(N, avg, idle, counts, dw, donors): the codes of ``kind`` are dead after this step, no other is"""
    N = rng.random(K, dtype=np.float32) * 5
    avg = rng.standard_normal((K, D)).astype(np.float32)
    counts = rng.integers(1, 40, K).astype(np.float32)
    dw = rng.standard_normal((K, D)).astype(np.float32) * counts[:, None]
    idle = rng.integers(0, 3 * P, K).astype(np.int32)              # (reset by counts > 0 wherever it is not overwritten below)
    quiet = rng.choice(K, max(K // 5, 1), replace=False)           # unused this step, but not for long enough
    counts[quiet], dw[quiet], idle[quiet] = 0.0, 0.0, rng.integers(0, P - 1, len(quiet))
    edges = [k for k in (0, 63, 64, 1023, 1024, K - 1) if 0 <= k < K]
    dead = {"none": [], "few": edges[:R - 1], "many": sorted(set(edges) | set(range(1, K, 7)) | set(range(max(K - 9, 0), K)))}[kind]
    for i, k in enumerate(dead):
        counts[k], dw[k] = 0.0, 0.0
        idle[k] = (P - 1, P + 3, INT32_MAX - 1, INT32_MAX)[i % 4]      # due now, overdue, about to saturate, saturated
    if kind == "many" and K > 4:
        idle[dead[-1]] = INT32_MAX       # beyond the cap: has to stay there
        assert len(dead) > R
    donor_rows = rng.standard_normal((R, D)).astype(np.float32)
    donor_rows[0, 0] = -0.0
    return N, avg, idle, counts, dw, donor_rows, dead


CASES = [(5, 8, "none", 4), (5, 8, "few", 4), (5, 8, "many", 2), (300, 8, "none", 8), (300, 8, "few", 8), (300, 8, "many", 8),
         (2051, 8, "none", 64), (2051, 8, "few", 64), (2051, 8, "many", 64), (2051, 8, "many", 1),
         (2048, 256, "none", 32), (2048, 256, "few", 32), (2048, 256, "many", 32)]


@pytest.mark.parametrize("K,D,kind,R", CASES)
def test_update_is_the_plain_update_on_substituted_inputs(K, D, kind, R):
    P = 3
    rng = np.random.default_rng(K * 131 + D + R)
    N, avg, idle, counts, dw, donor_rows, dead = _case(K, D, kind, R, P, rng)
    dev = _Device(N, avg, idle, K, D, R)
    for call in range(2):      # back to back on the same buffers: the second step has no assignment at all, so every quiet code ages too
        want_idle, want_info = ref.idle_rule(idle, counts, P, R)
        ids = want_info[2:2 + want_info[1]]
        if call == 0:
            assert want_info[0] == len(dead) and list(ids) == dead[:R]
            if kind == "none":      # nothing dead: the plain update on the SAME inputs
                assert want_info[1] == 0
        wN, wavg, wcb = _ema(*ref.substitute(N, avg, counts, dw, ids, donor_rows), K, D)
        gN, gavg, gcb, gidle, ginfo = dev.update(counts, dw, donor_rows, P)
        assert np.array_equal(ginfo, want_info), (call, ginfo[:8], want_info[:8])
        assert np.array_equal(gidle, want_idle), call
        for name, g, w in (("N", gN, wN), ("embed_avg", gavg, wavg), ("codebook", gcb, wcb)):
            assert np.array_equal(_bits(g), _bits(w)), (call, name, int((_bits(g) != _bits(w)).sum()))
        if call == 0 and kind == "many" and K > 4:
            assert gidle[dead[-1]] == INT32_MAX and gidle[dead[R]] >= P      # beyond the cap: still counting, saturated instead of wrapped
            assert np.array_equal(_bits(gN[ids]), _bits(np.full(len(ids), np.float32(1) - np.float32(DECAY))))
        N, avg, idle = gN, gavg, gidle
        counts, dw = np.zeros_like(counts), np.zeros_like(dw)
        donor_rows = rng.standard_normal((R, D)).astype(np.float32)


def test_bad_arguments_return_the_documented_codes():
    _ffi, lib, st = _lib()
    K, D, R = 16, 8, 4
    f = torch.zeros(K * D + 64, device="cuda")
    i = torch.zeros(K + 8, dtype=torch.int32, device="cuda")
    p, ip = _ffi.ptr(f), _ffi.ptr(i)
    good = dict(N=p, avg=p, cb=p, counts=p, dw=p, K=K, D=D, idle=ip, patience=1, donors=p, R=R, info=ip)

    def upd(**kw):
        a = dict(good, **kw)
        return lib.sa_vq_ema_update_restart(a["N"], a["avg"], a["cb"], a["counts"], a["dw"], a["K"], a["D"], DECAY, EPS, a["idle"], a["patience"], a["donors"],
                                            a["R"], a["info"], st)

    for bad in (dict(N=None), dict(avg=None), dict(cb=None), dict(counts=None), dict(dw=None), dict(idle=None), dict(donors=None), dict(info=None),
                dict(K=0), dict(D=0), dict(R=0), dict(R=65), dict(patience=0)):
        assert upd(**bad) == _ffi.SA_EINVAL, bad
    assert upd(D=12) == _ffi.SA_EUNSUPPORTED

    def gat(rows=p, M=8, D=8, base=0, Mtot=8, R=4, donors=p):
        return lib.sa_vq_restart_donors(rows, M, D, base, Mtot, R, 1, 2, donors, st)

    for bad in (dict(rows=None), dict(donors=None), dict(M=0), dict(D=0), dict(R=0), dict(R=65), dict(base=-1), dict(base=1), dict(Mtot=7)):
        assert gat(**bad) == _ffi.SA_EINVAL, bad
    assert gat(D=12) == _ffi.SA_EUNSUPPORTED
    assert gat() == 0 and upd() == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the module
K_Q, D_Q, P_Q, R_Q, SEED_Q = 16, 8, 2, 4, 4


def _quantizer(restart=True):
    from synthanatomy_amd.networks.vqvae.baseline import Quantizer
    torch.manual_seed(2)
    q = Quantizer(n_embed=K_Q, embed_dim=D_Q, decay=DECAY).cuda().train()
    if restart:
        q.impl.set_restart(P_Q, R_Q, SEED_Q)
    return q


def _clustered(q0_weight, step):
    """x [1, D, 4, 4, 4]: 64 rows within 0.01 of codes 3 and 9 of the INITIAL codebook"""
    g = torch.Generator().manual_seed(100 + step)
    which = torch.where(torch.rand(64, generator=g) < 0.5, 3, 9)
    rows = q0_weight[which] + 0.01 * torch.randn(64, D_Q, generator=g)
    return rows.reshape(1, 4, 4, 4, D_Q).permute(0, 4, 1, 2, 3).contiguous().cuda()


def _hand_made(q, x):
    """sa_vq_assign (+ sa_vq_stats_det: the deterministic switch is on) on the module's current codebook -> rows, counts, dw on the host"""
    _ffi, lib, st = _lib()
    rows = x.permute(0, 2, 3, 4, 1).contiguous()
    M = rows.numel() // D_Q
    cb = q.impl.weight.detach().clone()
    counts, dw, sq, wn, ws = (torch.zeros(n, device="cuda") for n in (K_Q, K_Q * D_Q, 1, K_Q, K_Q))
    idx, zq = torch.empty(M, dtype=torch.int64, device="cuda"), torch.empty_like(rows)
    _ffi.check(lib.sa_vq_assign(_ffi.ptr(rows), _ffi.ptr(cb), M, K_Q, D_Q, _ffi.ptr(idx), _ffi.ptr(zq), None, _ffi.ptr(counts), _ffi.ptr(dw), _ffi.ptr(sq),
                                _ffi.ptr(wn), st), "sa_vq_assign")
    _ffi.check(lib.sa_vq_stats_det(_ffi.ptr(rows), _ffi.ptr(cb), _ffi.ptr(idx), M, K_Q, D_Q, _ffi.ptr(counts), _ffi.ptr(dw), _ffi.ptr(sq), _ffi.ptr(ws), st),
               "sa_vq_stats_det")
    torch.cuda.synchronize()
    return rows.reshape(M, D_Q).cpu().numpy(), counts.cpu().numpy(), dw.reshape(K_Q, D_Q).cpu().numpy()


def _state(q):
    q.impl.wait_ema()
    torch.cuda.synchronize()
    out = {k: getattr(q.impl, k).detach().cpu().numpy().copy() for k in ("N", "embed_avg", "weight")}
    if q.impl._restart is not None:
        out["idle"] = q.impl.idle.cpu().numpy().copy()
    return out


@pytest.fixture()
def deterministic():
    from synthanatomy_amd import debug
    debug.set_deterministic(True)
    yield
    debug.set_deterministic(False)


def test_quantizer_restarts_dead_codes_from_rows_of_the_step(deterministic):
    q = _quantizer()
    w0 = q.impl.weight.detach().cpu().clone()
    assert "idle" not in q.state_dict() and len(q.state_dict()) == 4
    seen = []
    for step in range(5):
        x = _clustered(w0, step)
        before = _state(q)
        rows, counts, dw = _hand_made(q, x)
        if step < 2:      # (later the restarted codes sit on rows of the batch and are chosen too)
            assert sorted(np.flatnonzero(counts)) == [3, 9]
        q.impl._restart_step = step
        q(x)
        after = _state(q)
        info = q.impl.restart_info()
        want_idle, want_info = ref.idle_rule(before["idle"], counts, P_Q, R_Q)
        ids = list(want_info[2:2 + want_info[1]])
        assert (info["dead"], info["restarted"], info["ids"]) == (want_info[0], want_info[1], ids)
        donor_rows = ref.donors(rows, R_Q, SEED_Q, step)
        wN, wavg, wcb = _ema(*ref.substitute(before["N"], before["embed_avg"], counts, dw, ids, donor_rows), K_Q, D_Q)
        for name, w in (("N", wN), ("embed_avg", wavg), ("weight", wcb)):
            assert np.array_equal(_bits(after[name]), _bits(w)), (step, name)
        assert np.array_equal(after["idle"], want_idle)
        for i, k in enumerate(ids):      # a restarted code sits on its donor row (up to the eps smoothing of N)
            np.testing.assert_allclose(after["weight"][k], donor_rows[i], rtol=1e-3, atol=1e-6)
        seen.append((info["dead"], info["restarted"], info["ids"]))
    # patience 2: nothing at step 0; at step 1 the 14 codes nobody uses are dead and the first four restart, then the next four of the ten left
    assert seen[0] == (0, 0, []) and seen[1] == (14, 4, [0, 1, 2, 4]) and seen[2] == (10, 4, [5, 6, 7, 8])
    assert q.impl.restart_info()["total"] == sum(s[1] for s in seen)
    # eval never restarts and never touches idle
    before = _state(q)
    q.eval()
    q(_clustered(w0, 9))
    after = _state(q)
    assert all(np.array_equal(_bits(before[k]), _bits(after[k])) if k != "idle" else np.array_equal(before[k], after[k]) for k in before)
    assert q.impl.restart_info()["total"] == sum(s[1] for s in seen)


def test_feature_off_is_the_two_launch_step(deterministic):
    q = _quantizer(restart=False)
    w0 = q.impl.weight.detach().cpu().clone()
    for step in range(2):
        x = _clustered(w0, step)
        before = _state(q)
        _, counts, dw = _hand_made(q, x)
        q(x)
        after = _state(q)
        assert q.impl._stats.numel() == K_Q + K_Q * D_Q and not hasattr(q.impl, "idle")
        wN, wavg, wcb = _ema(before["N"], before["embed_avg"], counts, dw, K_Q, D_Q)
        for name, w in (("N", wN), ("embed_avg", wavg), ("weight", wcb)):
            assert np.array_equal(_bits(after[name]), _bits(w)), (step, name)
    with pytest.raises(RuntimeError, match="off"):
        q.impl.restart_info()


def test_resuming_equals_not_stopping(deterministic):
    from synthanatomy_amd.networks.vqvae.baseline import CodebookRestartState

    def steps(q, w0, lo, hi):
        for step in range(lo, hi):
            q.impl._restart_step = step
            q(_clustered(w0, step))

    a = _quantizer()
    w0 = a.impl.weight.detach().cpu().clone()
    steps(a, w0, 0, 4)
    b = _quantizer()
    steps(b, w0, 0, 2)
    net_sd = {k: v.cpu().clone() for k, v in b.state_dict().items()}
    extra = CodebookRestartState(b.impl).state_dict()
    assert sorted(extra) == ["idle", "max_per_step", "patience", "total"] and extra["idle"].dtype == torch.int32
    c = _quantizer()
    with torch.no_grad():
        c.impl.weight.normal_()      # (a fresh module with another codebook: everything has to come from the two state dicts)
    c.load_state_dict(net_sd)
    CodebookRestartState(c.impl).load_state_dict(extra)
    steps(c, w0, 2, 4)
    sa, sc = _state(a), _state(c)
    assert sa["idle"].any() and a.impl.restart_info()["total"] > 0
    for k in ("N", "embed_avg", "weight"):
        assert np.array_equal(_bits(sa[k]), _bits(sc[k])), k
    assert np.array_equal(sa["idle"], sc["idle"])
    assert a.impl.restart_info() == c.impl.restart_info()
