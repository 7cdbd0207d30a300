"""The optimiser apply (csrc/hip/kernels_apply.hip, the CPU backend's
table_apply) against a float32 model of the recurrence, bit for bit.

With the gradients given, an apply is a sequential float32 recurrence per (key,
parameter); the build is -ffp-contract=off so that it is the same floats on
every path.  xflow_amd/testing/apply_ref.py holds the model.  Each case plants
pre-states (import_table), drives s_pull + s_apply / s_apply_csr or push_host
with gradients chosen here, and compares export_table's words and the pulled
weights with the model's: assert_array_equal on uint32 views, no tolerance.
The one substitution: a never-pushed latent's lazy-init weight (logf, cosf) is
taken from the engine and held to hashing.normal_init within 4 ulp.

Every GPU case first asserts the kernels it reaches (apply_ref.apply_kernels
mirrors launch_table_apply); test_every_apply_kernel_is_covered asserts that
the cases' union is all of them.  The CSR routes and the compact (B, C) rows
exist on the GPU only: the CPU backend has neither, its variants of those
cases are left out (CSR) or run on full rows (reference FM).
"""
import numpy as np
import pytest
import torch

from xflow_amd.config import EngineConfig, ModelConfig, OptimConfig
from xflow_amd.engine import Engine
from xflow_amd.testing import apply_ref as ar
from xflow_amd.testing.hashing import fmix64, normal_init

F32 = np.float32
CPU = torch.device("cpu")
DEVICES = ["cpu", pytest.param("gpu", marks=pytest.mark.gpu)]
GPU_ONLY = [pytest.param("gpu", marks=pytest.mark.gpu)]
L1 = F32(OptimConfig().lambda1)
# key counts per launch: the packed groups' and the block's edges, and enough
# keys for several grid-stride iterations and several waves' deferral lists
NS = (1, 63, 64, 65, 255, 256, 257, 5000)
# chain lengths: the edges of kCsrShortChain (16), kCsrChunk (8), kCsrRowChunk
# (4), the short chains' chunks of 4 and the P-wide cooperative chunks
CHAINS = (0, 1, 2, 3, 4, 5, 8, 9, 15, 16, 17, 23, 24, 25, 32, 33)

CONFIGS = {   # name: (kind, opt, v_dim, fm_math)
    "lr-ftrl": ("lr", "ftrl", 1, "reference"), "lr-sgd": ("lr", "sgd", 1, "reference"),
    "fmref4": ("fm", "ftrl", 4, "reference"), "fmref8": ("fm", "ftrl", 8, "reference"),
    "fmref16": ("fm", "ftrl", 16, "reference"), "fmref3": ("fm", "ftrl", 3, "reference"),
    "fmref4-sgd": ("fm", "sgd", 4, "reference"),
    "fmstd4": ("fm", "ftrl", 4, "standard"), "fmstd8": ("fm", "ftrl", 8, "standard"),
    "fmstd16": ("fm", "ftrl", 16, "standard"), "fmstd3": ("fm", "ftrl", 3, "standard"),
    "mvm4": ("mvm", "ftrl", 4, "reference"), "mvm10": ("mvm", "ftrl", 10, "reference"),
    "mvm4-sgd": ("mvm", "sgd", 4, "reference"), "mvm10-sgd": ("mvm", "sgd", 10, "reference"),
}
CSR_CFGS = [c for c in CONFIGS if c != "lr-sgd"]   # (LR-SGD has no CSR apply)
# (device, route) pairs: the CPU backend has no CSR apply
_G = pytest.mark.gpu
ROUTES = [pytest.param("cpu", "dense1"), pytest.param("cpu", "dense8"),
          pytest.param("gpu", "dense1", marks=_G), pytest.param("gpu", "dense8", marks=_G),
          pytest.param("gpu", "csr", marks=_G)]
ROUTE_S = {"dense1": 1, "dense8": 8, "csr": 64}
LR16 = "k_apply_lr16"
GRP = "k_apply_group"
# the kernels each GPU case must reach, collected for test_every_apply_kernel_is_covered
COVERED = {}


@pytest.fixture
def device(request):
    if request.param == "cpu":
        return CPU
    return request.getfixturevalue("gpu_device")


def _bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def make_grads(rng, shape):
    """Gradients over six decades up to |g| = 1e3, with exact zeros, a
    denormal, 1e-20 (g * g underflows) and +-1e3 sprinkled in."""
    g = (rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 3, shape)).astype(F32)
    r = rng.random(shape)
    for lo, hi, v in ((0, .04, 0.0), (.04, .06, 1e-40), (.06, .08, 1e-20), (.08, .09, 1e3),
                      (.09, .10, -1e3), (.10, .11, -0.0)):
        g[(r >= lo) & (r < hi)] = F32(v)
    return g


def make_states(rng, L, m):
    """State words [m, W] that sit on the recipe's branches: z on +-lambda1 and
    the floats either side, z = -0.0, n = 0 with the flag set, n so large that
    sqrt(n + g * g) == sqrt(n); never-pushed latent keys (flag 0, zero state)."""
    inf = F32(np.inf)
    zs = np.array([L1, -L1, np.nextafter(L1, inf), np.nextafter(L1, F32(0)), np.nextafter(-L1, -inf),
                   np.nextafter(-L1, F32(0)), -0.0, 0.0, 3e-5, -9e-5, 0.01, -0.3, 2.0], dtype=F32)
    ns = np.array([0.0, 0.0, 0.25, 1.0, 7.0, 1e8, 3e10, 1e-30, 123.456], dtype=F32)
    st = np.zeros((m, L.P, L.sp), F32)
    if L.ftrl:
        st[:, :, 0] = rng.choice(ns, (m, L.P))
        st[:, :, 1] = rng.choice(zs, (m, L.P))
        r = rng.random((m, L.P)) < 0.3
        st[:, :, 1][r] = (rng.standard_normal((m, L.P)) * 0.05).astype(F32)[r]
    else:
        st[:, :, 0] = rng.choice(np.array([0.0, -0.0, 1e-3, 0.5, -0.25], dtype=F32), (m, L.P))
    words = np.zeros((m, L.W), np.uint32)
    flag = np.ones(m, np.uint32)
    if L.has_flag:
        flag[rng.random(m) < 0.3] = 0
        st[flag == 0] = 0
        words[:, L.flag_col] = flag
    words[:, :L.sp * L.P] = st.reshape(m, -1).view(np.uint32)
    return words


class Ctx:
    """One engine with its model; keys come from a universe fixed up front."""

    def __init__(self, device, cfg, n_keys, S=1, seed=0, **ecfg):
        kind, opt, v_dim, math = CONFIGS[cfg]
        self.L = ar.Layout(kind, opt, v_dim, math)
        self.device, self.gpu = device, device.type == "cuda"
        self.rng = np.random.default_rng(seed)
        self.optim = OptimConfig(kind=opt)
        log2 = max(10, int(np.ceil(np.log2(n_keys * 2.5))))
        self.eng = Engine(ModelConfig(kind=kind, v_dim=v_dim, fm_math=math), self.optim,
                          EngineConfig(table_log2_cap=log2, max_rows=256, max_nnz=2048,
                                       max_slices=S, **ecfg), device=device)
        L = self.L
        assert self.eng.state_words == L.W
        if self.gpu:
            assert self.eng.pstride == L.pstride
        L.pstride = self.eng.pstride   # (the CPU backend does not pad the latent width)
        assert self.eng.params_per_key == L.P
        self.compact = self.gpu and L.compact_ok
        assert self.eng.grad_width == (2 if self.compact else L.pstride)
        self.universe = np.unique(fmix64(np.arange(1, n_keys + 1, dtype=np.uint64) +
                                         np.uint64((seed + 1) << 24)))
        assert len(self.universe) == n_keys
        lazy = ar.lazy_weights(self.eng, self.universe)
        self.model = ar.ApplyModel(L, self.optim, self.universe, lazy)
        self.free = self.rng.permutation(n_keys)     # universe indices not handed out yet

    def take(self, n):
        idx, self.free = np.sort(self.free[:n]), self.free[n:]
        assert len(idx) == n, "universe too small"
        return idx

    def plant(self, idx):
        words = make_states(self.rng, self.L, len(idx))
        self.eng.import_table(self.universe[idx], words.reshape(-1))
        self.model.plant(idx, words)

    def tensor(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def check(self, start=None):
        """Exported words and pulled weights equal the model's."""
        m, L = self.model, self.L
        k, w = self.eng.export_table()
        o = np.argsort(k)
        k, w = k[o], np.asarray(w, dtype=np.uint32).reshape(len(k), L.W)[o]
        live = np.nonzero(m.present)[0]
        np.testing.assert_array_equal(k, self.universe[live], err_msg="keys in the table")
        want = m.words(live)
        if not np.array_equal(w, want):
            bad = np.argwhere(w != want)
            lines = []
            for r, c in bad[:6]:
                p = min(int(c) // L.sp, L.P - 1)
                where = (m.explain(start, k[r], p, w[r]) if start is not None and c < L.sp * L.P
                         else f"key {int(k[r]):#x} word {c}: model {want[r, c]:#x} device {w[r, c]:#x}")
                lines.append(where)
            raise AssertionError(f"{len(bad)} state words of {len(np.unique(bad[:, 0]))} keys differ:\n"
                                 + "\n".join(lines))
        got = np.asarray(self.eng.pull(self.universe), dtype=F32).reshape(-1, L.P)
        np.testing.assert_array_equal(_bits(got), _bits(m.weights()), err_msg="pulled weights")
        assert not self.eng.overflowed()


class Call:
    """One s_pull + apply of ``srcs`` (per source: universe indices, unique
    inside a source) with S slices."""

    def __init__(self, T, srcs, S, *, masks=False, csr=False, mode="mix", buf=0, insert=True,
                 keep_weights=False, sum_slices=False, apply_offsets=None, pull_offsets=True):
        self.T, self.S, self.masks, self.csr, self.buf = T, S, masks, csr, buf
        self.insert, self.keep, self.sum = insert, keep_weights, sum_slices
        L, rng = T.L, T.rng
        self.srcs = [np.asarray(s, dtype=np.int64) for s in srcs]
        self.idx = np.concatenate(self.srcs) if srcs else np.zeros(0, np.int64)
        self.n = len(self.idx)
        self.offsets = [0] + list(np.cumsum([len(s) for s in self.srcs]))
        self.apply_offsets = self.offsets if apply_offsets is None else apply_offsets
        self.pull_offsets = self.offsets if pull_offsets else None
        n, gw = self.n, T.eng.grad_width
        self.compact = T.compact
        # chain lengths and the slices they sit in (ascending)
        if S == 1 and not masks and not csr:
            cnt = np.ones(n, np.int64)
        elif sum_slices:
            cnt = np.full(n, S, np.int64)
        else:
            pool = {"mix": [c for c in CHAINS if c <= S] + [S],
                    "long": [c for c in CHAINS if ar.CSR_SHORT_CHAIN < c <= S] + [S],
                    "short": [c for c in CHAINS if c <= min(S, ar.CSR_SHORT_CHAIN)]}[mode]
            cnt = rng.choice(np.array(pool), n)
        self.cnt = cnt
        sl = np.argsort(rng.random((n, S)), axis=1)          # a random subset of cnt slices
        pick = np.arange(S)[None, :] < cnt[:, None]
        if n > 4 and masks:                                   # single bits: the lowest and the highest
            cnt[0], cnt[1], cnt[2], cnt[3] = 1, 1, 0, S   # ... an empty mask, all bits
            pick = np.arange(S)[None, :] < cnt[:, None]
            sl[0], sl[1] = np.arange(S), np.arange(S)[::-1]
        self.bits = np.zeros((n, S), bool)
        np.put_along_axis(self.bits, sl, pick, axis=1)
        assert (self.bits.sum(1) == cnt).all()
        self.mask = (self.bits * (1 << np.arange(S, dtype=np.uint64))).sum(1).astype(np.uint32) \
            if S <= 32 else None
        # gradients for every (entry, slice): the slices outside the chain hold
        # values too, which the apply must not read
        width = 2 if self.compact else L.P
        self.g = make_grads(rng, (n, S, width))
        # a chain that drives z through the L1 dead zone and out (z0 = -9e-5 is
        # among the planted values): equal pushes of +6e-5
        walk = (np.arange(n) % 11 == 5) & (cnt >= 4)
        self.g[walk] = F32(6e-5) / (F32(L.v_dim) if self.compact else F32(1))
        order = np.argsort(~self.bits, axis=1, kind="stable")  # chain j -> slice
        self.chain = np.take_along_axis(self.g, order[:, :, None], axis=1)   # [n, S, width]

    # the kernels launch_table_apply picks for this call
    def kernels(self, grouped=False, stash=False):
        return ar.apply_kernels(self.T.L, gpu=self.T.gpu, S=self.S, masks=self.masks, csr=self.csr,
                                grouped=grouped, stash=stash, sum_slices=self.sum)

    def pull(self):
        T, L = self.T, self.T.L
        self.keys_t = T.tensor(T.universe[self.idx].view(np.int64))
        vals = torch.full((max(self.n, 1), T.eng.value_width), 7.0, dtype=torch.float32, device=T.device)
        kw = {} if self.pull_offsets is None else {"offsets": self.pull_offsets}
        T.eng.s_pull(self.keys_t, self.n, vals, insert=self.insert, buf=self.buf,
                     keep_weights=self.keep, **kw)
        if self.insert:
            T.model.insert(self.idx)
        self.w_pull = T.model.weights(self.idx)
        v = vals.cpu().numpy()[:self.n]
        if T.eng.value_width == L.pstride:     # (compact value rows: (w, sum v, sum v^2, 0))
            np.testing.assert_array_equal(_bits(v[:, :L.P]), _bits(self.w_pull), err_msg="s_pull")
            if T.gpu:   # (the CPU pull leaves the padding alone)
                assert (_bits(v[:, L.P:]) == 0).all(), "padding of the pulled rows"
        else:
            np.testing.assert_array_equal(_bits(v[:, 0]), _bits(self.w_pull[:, 0]), err_msg="s_pull")

    def apply(self):
        T, L, S = self.T, self.T.L, self.S
        eng, m = T.eng, T.model
        active = sum(len(s) > 0 for s in self.srcs)
        if self.csr:
            ew = 2 if L.kind == "lr" else (3 if self.compact else ar.csr_row_words(L.P))
            tot = int(self.cnt.sum())
            ent = np.zeros((tot + 1, ew), np.uint32)
            rows = np.repeat(np.arange(self.n), self.cnt)
            j = np.arange(tot) - np.repeat(np.cumsum(self.cnt) - self.cnt, self.cnt)
            slices = np.sort(np.where(self.bits, np.arange(S)[None, :], S), axis=1)
            ent[:tot, 0] = slices[rows, j]
            ent[:tot, 1:1 + self.chain.shape[2]] = _bits(self.chain[rows, j])
            self.dev = (T.tensor(self.cnt.astype(np.uint32).view(np.int32)), T.tensor(ent.view(np.int32)))
            eng._sync_stream()
            eng.native.s_apply_csr(self.keys_t.data_ptr(), self.dev[0].data_ptr(),
                                   self.dev[1].data_ptr(), [int(o) for o in self.offsets], S, self.buf)
        else:
            gw = eng.grad_width
            dense = make_grads(T.rng, (self.n, S, gw))     # (the padded columns hold values too)
            dense[:, :, :self.g.shape[2]] = self.g
            mt = T.tensor(self.mask.view(np.int32)) if self.masks else None
            self.dev = (T.tensor(dense), mt)
            eng.s_apply(self.keys_t, self.dev[0], mt, [int(o) for o in self.apply_offsets], S,
                        buf=self.buf)
        # the model: the sources' launches in order
        for s, src in enumerate(self.srcs):
            if not len(src):
                continue
            lo, hi = self.offsets[s], self.offsets[s + 1]
            chain, cnt = self.chain[lo:hi], self.cnt[lo:hi]
            if self.sum:
                acc = np.zeros_like(chain[:, 0])
                with np.errstate(all="ignore"):
                    for j in range(S):
                        acc = acc + chain[:, j]
                chain, cnt = acc[:, None, :], np.ones(hi - lo, np.int64)
            if self.compact:
                # the pre-step weights: the pull's where the engine kept them
                # (keep_weights, or several sources: s_pull keeps them itself)
                w_pre = self.w_pull[lo:hi] if (self.keep or active > 1) else m.weights(src)
                m.launch(src, cnt=cnt, bc=chain, w_pre=w_pre)
            else:
                m.launch(src, g=chain, cnt=cnt)


def _expect(call, names, **kw):
    """The case reaches exactly these kernels (GPU; the CPU backend has one apply)."""
    got = call.kernels(**kw)
    if call.T.gpu:
        assert got == frozenset(names), got
    else:
        assert got == frozenset({"cpu"})


# --------------------------------------------------------------- the model itself
def _ulps(a, b):
    """Distance of two float32 arrays in units in the last place (ordered ints)."""
    def o(x):
        i = np.ascontiguousarray(x, dtype=F32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(o(a) - o(b))


@pytest.mark.parametrize("device", DEVICES, indirect=True)
@pytest.mark.parametrize("cfg", ["fmref16", "mvm10", "fmref4-sgd"])
def test_lazy_init_within_4_ulp(device, cfg):
    """The lazy init the model borrows from the engine (logf, cosf: not bit
    for bit numpy's) is hashing.normal_init * v_init_scale within 4 ulp, w's
    is 0, SGD's is sgd_v_init exactly."""
    T = Ctx(device, cfg, 6000, seed=23)
    L, lazy = T.L, T.model.lazy
    assert (_bits(lazy[:, :L.p_w]) == 0).all()
    worst = 0
    for p in range(L.p_w, L.P):
        if L.ftrl:
            want = normal_init(T.universe, p - L.p_w, T.optim.seed) * F32(T.optim.v_init_scale)
            d = _ulps(lazy[:, p], want)
            worst = max(worst, int(d.max()))
            print(f"latent {p}: max {int(d.max())} ulp, {int((d > 4).sum())} of {len(d)} above 4")
        else:
            assert (lazy[:, p] == F32(T.optim.sgd_v_init)).all()
    assert worst <= 4, f"lazy init {worst} ulp from hashing.normal_init"
def test_model_dead_zone_walk():
    """The recipe on the branch edges: a chain of equal pushes takes z from
    below -lambda1 through the dead zone (weight exactly 0) and out again."""
    L = ar.Layout("lr", "ftrl")
    m = ar.ApplyModel(L, OptimConfig(), np.array([5], np.uint64), np.zeros((1, 1), F32))
    w = np.zeros((1, L.W), np.uint32)
    w[0, :2] = np.array([0.0, -9e-5], F32).view(np.uint32)
    m.plant(np.array([0]), w)
    ws = [float(m.weights()[0, 0])]
    for _ in range(3):
        m.launch(np.array([0]), g=np.full((1, 1, 1), 6e-5, F32), cnt=np.array([1]))
        ws.append(float(m.weights()[0, 0]))
    assert ws[0] > 0 and ws[1] == 0 and ws[2] == 0 and ws[3] < 0
    # z exactly on +-lambda1 is inside, the next float is outside
    for z, zero in ((L1, True), (-L1, True), (np.nextafter(L1, F32(1)), False),
                    (np.nextafter(-L1, F32(-1)), False), (F32(-0.0), True)):
        assert (m._ftrl_weight(np.array([z], F32), np.array([1.0], F32))[0] == 0) == zero
    # n so large that a push leaves sqrt(n) unchanged: the proximal term is exactly 0
    assert np.sqrt(F32(1e8) + F32(3.0) * F32(3.0)) == np.sqrt(F32(1e8))


def test_dispatch_mirror_names():
    """apply_kernels names only real instantiations, and each is reachable."""
    seen = set()
    for cfg in CONFIGS:
        L = ar.Layout(*CONFIGS[cfg])
        for S in (1, 8, 64):
            for masks in (False, True):
                for grouped in (False, True):
                    seen |= ar.apply_kernels(L, gpu=True, S=S, masks=masks, grouped=grouped)
            if cfg in CSR_CFGS:
                seen |= ar.apply_kernels(L, gpu=True, S=S, masks=False, csr=True)
    assert seen == ar.ALL_KERNELS


# ------------------------------------------------------- one source, every count
def _rounds(T, S, expect, ns=NS, **kw):
    for n in ns:
        idx = T.take(n + 3)
        touched, by = T.rng.permutation(idx[:n]), idx[n:]
        T.plant(np.concatenate([touched[::2], by]))       # every other key is new to the table
        start = T.model.copy()
        c = Call(T, [touched], S, **kw)
        _expect(c, expect, stash=T.gpu and T.L.kind == "lr" and T.L.ftrl)
        c.pull()
        c.apply()
        T.check(start)                                     # (the bystanders: bit-unchanged)


@pytest.mark.parametrize("device", DEVICES, indirect=True)
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_one_slice(device, cfg):
    """S = 1, no masks: k_apply_lr16<false>, k_apply_group<false> (the gradient
    row in the pipeline), k_apply_generic (LR-SGD)."""
    T = Ctx(device, cfg, sum(NS) + 3 * len(NS), seed=1)
    name = {"lr-ftrl": f"{LR16}<false>", "lr-sgd": "k_apply_generic"}.get(cfg, f"{GRP}<false>")
    COVERED[("one_slice", cfg)] = {name}
    _rounds(T, 1, {name})


@pytest.mark.parametrize("device", DEVICES, indirect=True)
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_slice_masks(device, cfg):
    """S = 8 with slice masks (empty, single-bit, all bits among them), the
    pushes in ascending slice order: k_apply_lr16<true>, k_apply_group<true>."""
    T = Ctx(device, cfg, sum(NS) + 3 * len(NS), S=8, seed=2)
    name = {"lr-ftrl": f"{LR16}<true>", "lr-sgd": "k_apply_generic"}.get(cfg, f"{GRP}<true>")
    COVERED[("slice_masks", cfg)] = {name}
    _rounds(T, 8, {name}, masks=True)


@pytest.mark.parametrize("device", DEVICES, indirect=True)
@pytest.mark.parametrize("cfg", ["lr-ftrl", "fmref4", "mvm10-sgd"])
def test_mask_bit_31(device, cfg):
    """S = 32: bit 31 alone, all 32 bits (the `all` mask's S >= 32 branch)."""
    T = Ctx(device, cfg, 400, S=32, seed=3)
    name = {"lr-ftrl": f"{LR16}<true>"}.get(cfg, f"{GRP}<true>")
    _rounds(T, 32, {name}, ns=(65, 257), masks=True)


@pytest.mark.parametrize("device", DEVICES, indirect=True)
@pytest.mark.parametrize("cfg", ["lr-ftrl", "lr-sgd", "fmstd4", "mvm4"])
def test_sum_slices(device, cfg):
    """sum_slices: one push of the float32 sum accumulated in slice order.
    LR-FTRL with the pull's stash runs on k_apply_group<true> with P = 1."""
    T = Ctx(device, cfg, 700, S=8, seed=4, sum_slices=True)
    name = "k_apply_generic" if cfg == "lr-sgd" else f"{GRP}<true>"
    COVERED[("sum_slices", cfg)] = {name}
    _rounds(T, 8, {name}, ns=(1, 65, 257), sum_slices=True)


def _csr_names(cfg, long):
    L = ar.Layout(*CONFIGS[cfg])
    if L.kind == "lr":
        return {"k_apply_lr16_csr<false>"} | ({"k_apply_lr16_csr<true>"} if long else set())
    r = "false" if L.compact_ok else "true"
    return {f"k_apply_group_csr<false,{r}>"} | ({f"k_apply_group_csr<true,{r}>"} if long else set())


@pytest.mark.parametrize("device", GPU_ONLY, indirect=True)
@pytest.mark.parametrize("cfg", CSR_CFGS)
def test_csr_chains(device, cfg):
    """CSR entries, S = 64 (csr_long live): long and short chains mixed inside
    a wave, every count's edges; the deferred keys' second pass.  GPU only: the
    CPU backend has no CSR apply."""
    T = Ctx(device, cfg, sum(NS) + 3 * len(NS), S=64, seed=5)
    COVERED[("csr", cfg)] = _csr_names(cfg, True)
    _rounds(T, 64, _csr_names(cfg, True), csr=True)


@pytest.mark.parametrize("device", GPU_ONLY, indirect=True)
@pytest.mark.parametrize("mode", ["long", "short"])
@pytest.mark.parametrize("cfg", ["lr-ftrl", "fmref8", "fmstd4", "mvm10"])
def test_csr_all_long_or_none(device, cfg, mode):
    """Every key deferred, and none (empty deferral lists); S = 8 keeps csr_long off."""
    T = Ctx(device, cfg, 1200, S=64, seed=6)
    _rounds(T, 64, _csr_names(cfg, True), ns=(65, 257), csr=True, mode=mode)
    if mode == "short":
        _rounds(T, 8, _csr_names(cfg, False), ns=(65, 257), csr=True)


# ------------------------------------------------------------- several sources
def _three_sources(T, n, empty_middle=False):
    """Keys sent by 1, 2 and 3 of three sources (the leader is the first sender)."""
    idx = T.take(n)
    T.plant(idx[::2])
    who = T.rng.integers(1, 8, n)                         # bit s: source s sends the key
    if empty_middle:
        who = (who & 5) | ((who & 5) == 0)
    return [T.rng.permutation(idx[(who >> s) & 1 == 1]) for s in range(3)]


@pytest.mark.parametrize("device", DEVICES, indirect=True)
@pytest.mark.parametrize("empty_middle", [False, True])
@pytest.mark.parametrize("S", [1, 8])
@pytest.mark.parametrize("cfg", ["lr-ftrl", "fmref4", "fmref8", "fmstd16", "mvm10", "mvm4-sgd"])
def test_grouped_sources(device, cfg, S, empty_middle):
    """owner_group = 1: one launch, the leader entry applies every source's
    pushes in source order (k_apply_lr16_multi, k_apply_group with grp).  A
    latent's first push may come from a later source only (an earlier one sent
    an empty mask): the flag and the lazy init follow the first real push."""
    T = Ctx(device, cfg, 1400, S=S, seed=7 + S, owner_group=1)
    for n in (65, 600):
        srcs = _three_sources(T, n, empty_middle)
        start = T.model.copy()
        c = Call(T, srcs, S, masks=S > 1)
        grouped = T.gpu
        name = "k_apply_lr16_multi" if (cfg == "lr-ftrl" and S == 1) else f"{GRP}<{'true' if S > 1 else 'false'}>"
        if cfg == "lr-ftrl" and S == 1:
            COVERED[("grouped", cfg)] = {name}
        _expect(c, {name}, grouped=grouped)
        c.pull()
        c.apply()
        T.check(start)


@pytest.mark.parametrize("device,route", [r for r in ROUTES if r.values[1] != "dense1"],
                         indirect=["device"])
@pytest.mark.parametrize("cfg", ["lr-ftrl", "fmref4", "fmstd8", "mvm10"])
def test_source_by_source(device, cfg, route):
    """The grouping skipped: s_apply with offsets that differ from the pull's
    (the empty middle source dropped) and s_apply_csr run one launch per
    source in source order; only the first takes the stash.  Compact FM rows
    expand with the pull's weights for every source (keep_weights: the grouping
    was made, so s_pull did not keep them by itself)."""
    csr, S = route == "csr", ROUTE_S[route]
    T = Ctx(device, cfg, 1400, S=S, seed=11, owner_group=1)
    for n in (65, 600):
        srcs = _three_sources(T, n, empty_middle=True)
        start = T.model.copy()
        c = Call(T, srcs, S, masks=not csr, csr=csr, keep_weights=True)
        if not csr:   # drop the empty source: no longer the grouping's offsets
            c.apply_offsets = [c.offsets[0], c.offsets[1], c.offsets[3]]
            c.srcs = [c.srcs[0], c.srcs[2]]
            c.offsets = c.apply_offsets
            c.pull_offsets = [0, len(srcs[0]), len(srcs[0]), c.n]
        c.pull()
        c.apply()
        T.check(start)


# ------------------------------------------------------------------ the stash
@pytest.mark.parametrize("device,route", ROUTES, indirect=["device"])
@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("cfg", ["lr-ftrl", "fmref4", "mvm4"])
def test_stale_stash(device, cfg, route, keep):
    """Two buffers pull overlapping keys; the second applies first, so the
    first one's stash is stale and its apply reads the table.  keep_weights:
    compact FM rows still expand with the weights their pull saw."""
    S = ROUTE_S[route]
    T = Ctx(device, cfg, 900, S=S, seed=13)
    idx = T.take(600)
    T.plant(idx[::2])
    start = T.model.copy()
    kw = dict(masks=route == "dense8", csr=route == "csr", keep_weights=keep)
    a = Call(T, [idx[:400]], S, buf=0, **kw)
    b = Call(T, [idx[200:]], S, buf=1, **kw)
    a.pull()
    b.pull()
    b.apply()
    a.apply()
    T.check(start)


# --------------------------------------------------------------------- no slot
@pytest.mark.parametrize("device,route", ROUTES, indirect=["device"])
@pytest.mark.parametrize("cfg", ["lr-ftrl", "fmref8", "fmstd4", "mvm10", "mvm4-sgd"])
def test_lookup_only_pull_changes_nothing_absent(device, cfg, route):
    """A lookup-only s_pull leaves absent keys without a slot; the apply skips
    them (nothing inserted, nothing written) and pushes the present ones."""
    S = ROUTE_S[route]
    T = Ctx(device, cfg, 500, S=S, seed=17)
    idx = T.take(300)
    T.plant(idx[::3])
    start = T.model.copy()
    c = Call(T, [idx], S, masks=route == "dense8", csr=route == "csr", insert=False)
    c.pull()
    assert (T.eng.server_slots(0)[:c.n][~T.model.present[idx]] == ar.NO_SLOT).all()
    c.apply()
    assert T.eng.table_size() == len(idx[::3])
    T.check(start)


# ------------------------------------------------------------------- push_host
@pytest.mark.parametrize("device", DEVICES, indirect=True)
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_push_host(device, cfg):
    """Engine.push: one launch per key on P-wide rows, repeated keys in order."""
    T = Ctx(device, cfg, 200, seed=19)
    L = T.L
    idx = T.take(65)
    T.plant(idx[::2])
    start = T.model.copy()
    seq = np.concatenate([idx, idx[:9], idx[:3]])
    g = make_grads(T.rng, (len(seq), L.P))
    got = ar.apply_kernels(L, gpu=T.gpu, S=1, masks=False, pstride=L.P)
    name = f"{LR16}<false>" if cfg == "lr-ftrl" else (f"{GRP}<false>" if L.P >= 2 else "k_apply_generic")
    assert got == (frozenset({name}) if T.gpu else frozenset({"cpu"}))
    T.eng.push(T.universe[seq], g)
    T.model.insert(idx)
    for i, k in enumerate(seq):
        T.model.launch(np.array([k]), g=g[i][None, None, :], cnt=np.array([1]))
    T.check(start)


# --------------------------------------------------------------------- coverage
def test_every_apply_kernel_is_covered():
    """The union of what the cases above assert they reach is every apply
    kernel launch_table_apply can launch."""
    cases = {}
    for cfg in CONFIGS:
        L = ar.Layout(*CONFIGS[cfg])
        lrf = L.kind == "lr" and L.ftrl
        cases[("one_slice", cfg)] = ar.apply_kernels(L, gpu=True, S=1, masks=False, stash=lrf)
        cases[("slice_masks", cfg)] = ar.apply_kernels(L, gpu=True, S=8, masks=True, stash=lrf)
        if cfg in CSR_CFGS:
            cases[("csr", cfg)] = ar.apply_kernels(L, gpu=True, S=64, masks=False, csr=True)
    L = ar.Layout(*CONFIGS["lr-ftrl"])
    cases[("grouped", "lr-ftrl")] = ar.apply_kernels(L, gpu=True, S=1, masks=False, grouped=True)
    reached = frozenset().union(*cases.values())
    assert reached == ar.ALL_KERNELS, sorted(ar.ALL_KERNELS - reached)
    # ... and where those cases ran in this session, what they asserted is the same
    for k, names in COVERED.items():
        if k in cases:
            assert frozenset(names) == cases[k], k
