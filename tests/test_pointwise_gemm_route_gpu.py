"""Pointwise (1x1 / stride-1) convs on the gemm8p core: the forward with the
BatchNorm statistics epilogue and the dgrad with the ReLU-backward mask, every
tile the router can pick forced one at a time, against fp32 torch on the bf16
inputs. Tolerances are those of test_kernels_gpu.py::test_pointwise_conv_kernel
(1e-2 on outputs against fp32 torch, 1e-5 on the sums against the kernel's own
stored bf16 output in fp64).

The mask is the layout gemm_pw_kernel's dgrad epilogue reads: the bf16 ReLU
output itself (zero where it is <= 0), pitch ``ldm`` in elements."""
import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SHAPES = [(3136, 512, 2048), (200, 128, 512), (1000, 256, 1024)]     # (M, K, N)
TILES = [64, 128, 65, 129, 256]
# every (shape, tile) the router can pick: the 256^2 tile needs M, N >= 256
CASES = [(M, K, N, t) for (M, K, N) in SHAPES for t in TILES if t != 256 or (M >= 256 and N >= 256)]


def rel_err(a, b):
    a = a.float()
    b = b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def T():
    return torch.ops.tam


@pytest.fixture(autouse=True)
def _routed(gpu):
    yield
    T().conv_pw_gemm_policy(1, 0)
    T().gemm8p_policy(1, 0)


_cache = {}


def case(gpu, M, K, N):
    """Inputs and the fp32 references of one shape, computed once."""
    key = (M, K, N)
    if key not in _cache:
        g = torch.Generator(device=gpu).manual_seed(M + K + N)
        x = torch.randn(1, M, 1, K, device=gpu, generator=g).to(BF)
        w = (torch.randn(N, 1, 1, K, device=gpu, generator=g) / K ** 0.5).to(BF)
        ref = x.float().reshape(M, K) @ w.float().reshape(N, K).t()
        # dgrad of the transposed conv shape: dX[M][N] = dY[M][K] . Wd[K][N], Wd = a [K][1][1][N] weight
        wd = (torch.randn(K, 1, 1, N, device=gpu, generator=g) / K ** 0.5).to(BF)
        mask = torch.randn(1, M, 1, N, device=gpu, generator=g).to(BF)
        dref = (x.float().reshape(M, K) @ wd.float().reshape(K, N)) * (mask.float().reshape(M, N) > 0)
        _cache[key] = (x, w, ref, wd, mask, dref)
    return _cache[key]


def fwd(gpu, x, w, M, N, relu=False):
    from tiresias_amd.ops.functional import BN_SHARDS
    y = torch.empty(1, M, 1, N, device=gpu, dtype=BF)
    sums = torch.zeros(BN_SHARDS * 2 * N, device=gpu, dtype=torch.float64)
    done = T().conv_fwd(x, w, y, 1, 0, 1, None, relu, sums)
    torch.cuda.synchronize()
    return y.reshape(M, N), sums.view(BN_SHARDS, 2 * N).sum(0), done


def dgrad(gpu, dy, wd, mask, M, N):
    dx = torch.empty(1, M, 1, N, device=gpu, dtype=BF)
    wt = torch.empty_like(wd)
    T().conv_dgrad(dy, wd, wt, dx, 1, 0, 1, mask)
    torch.cuda.synchronize()
    return dx.reshape(M, N)


@pytest.mark.parametrize("M,K,N,tile", CASES)
def test_forward_stats(gpu, M, K, N, tile):
    x, w, ref, _, _, _ = case(gpu, M, K, N)
    T().conv_pw_gemm_policy(2, tile)
    y, tot, done = fwd(gpu, x, w, M, N)
    assert done == 1, "the gemm8p route computes the BN statistics"
    e_y = rel_err(y, ref)
    yd = y.double()
    e_s, e_q = rel_err(tot[:N], yd.sum(0)), rel_err(tot[N:], (yd * yd).sum(0))
    rd = ref.double()
    l_s, l_q = rel_err(tot[:N], rd.sum(0)), rel_err(tot[N:], (rd * rd).sum(0))
    print(f"fwd M={M} K={K} N={N} tile={tile}: y {e_y:.2e} sums own {e_s:.2e} {e_q:.2e} vs fp32 {l_s:.2e} {l_q:.2e}")
    assert e_y < 1e-2
    assert e_s < 1e-5 and e_q < 1e-5      # rows past M leak nothing, nothing counted twice
    assert l_s < 1e-2 and l_q < 1e-2


@pytest.mark.parametrize("tile", [64, 129])
def test_forward_stats_relu(gpu, tile):
    """stats + relu: the sums are of the stored (clamped) values."""
    M, K, N = SHAPES[2]
    x, w, ref, _, _, _ = case(gpu, M, K, N)
    T().conv_pw_gemm_policy(2, tile)
    y, tot, done = fwd(gpu, x, w, M, N, relu=True)
    assert done == 1 and rel_err(y, ref.clamp_min(0)) < 1e-2
    yd = y.double()
    assert rel_err(tot[:N], yd.sum(0)) < 1e-5 and rel_err(tot[N:], (yd * yd).sum(0)) < 1e-5


@pytest.mark.parametrize("M,K,N,tile", CASES)
def test_dgrad_mask(gpu, M, K, N, tile):
    x, _, _, wd, mask, dref = case(gpu, M, K, N)
    T().conv_pw_gemm_policy(2, tile)
    dx = dgrad(gpu, x, wd, mask, M, N)
    off = mask.reshape(M, N).float() <= 0
    assert rel_err(dx, dref) < 1e-2
    assert (dx[off] == 0).all(), "masked-out entries are exactly zero"
    # the same product as a plain gemm8p call on that tile with a mask pitch
    # ldm > N (the mask a column slice of a wider tensor)
    wide = torch.randn(M, N + 64, device=gpu).to(BF)
    wide[:, :N] = mask.reshape(M, N)
    mk = wide[:, :N]
    assert mk.stride(0) == N + 64
    wt = wd.reshape(K, N).t().contiguous()
    out = torch.empty(M, N, device=gpu, dtype=BF)
    T().gemm8p_policy(2, tile)
    T().gemm(x.reshape(M, K), True, wt, True, out, 0, None, False, mk, 1.0, False)
    torch.cuda.synchronize()
    assert rel_err(out, dref) < 1e-2
    assert (out[off] == 0).all()
    assert torch.equal(out, dx), "pitch of the mask changes nothing"


@pytest.mark.parametrize("M,K,N", SHAPES)
def test_off_switch(gpu, M, K, N):
    """TAM_CONV_PW_GEMM=0 (conv_pw_gemm_policy(0)): the conv core's results,
    within the same tolerances."""
    x, w, ref, wd, mask, dref = case(gpu, M, K, N)
    T().conv_pw_gemm_policy(0, 0)
    y, tot, done = fwd(gpu, x, w, M, N)
    assert rel_err(y, ref) < 1e-2
    if done:
        yd = y.double()
        assert rel_err(tot[:N], yd.sum(0)) < 1e-5 and rel_err(tot[N:], (yd * yd).sum(0)) < 1e-5
    dx0 = dgrad(gpu, x, wd, mask, M, N)
    assert rel_err(dx0, dref) < 1e-2
    T().conv_pw_gemm_policy(2, 128)
    y1, _, _ = fwd(gpu, x, w, M, N)
    dx1 = dgrad(gpu, x, wd, mask, M, N)
    assert rel_err(y1, y) < 1e-2 and rel_err(dx1, dx0) < 1e-2


def test_plain_epilogue_unchanged(gpu):
    """A gemm8p call without the new epilogues launches the unchanged
    instantiation: the conv route's plain store (stats off, mask off) is
    bit-identical to the plain gemm op on the same tile, and the stats
    variant stores the same bits as the plain one."""
    M, K, N = SHAPES[2]
    x, w, _, _, _, _ = case(gpu, M, K, N)
    for tile in TILES:
        T().conv_pw_gemm_policy(2, tile)
        y_plain = torch.empty(1, M, 1, N, device=gpu, dtype=BF)
        T().conv_fwd(x, w, y_plain, 1, 0, 1, None, False, None)
        y_stats, _, _ = fwd(gpu, x, w, M, N)
        out = torch.empty(M, N, device=gpu, dtype=BF)
        T().gemm8p_policy(2, tile)
        T().gemm(x.reshape(M, K), True, w.reshape(N, K), True, out, 0, None, False, None, 1.0, False)
        torch.cuda.synchronize()
        assert torch.equal(out, y_plain.reshape(M, N)), tile
        assert torch.equal(y_stats, y_plain.reshape(M, N)), tile


def test_route_table_roundtrip(gpu):
    """A shipped PW line routes the shape; an unmeasured shape is timed once
    outside capture and lands in gemm_routes()."""
    M, K, N = 1000, 256, 1024
    x, w, ref, _, _, _ = case(gpu, M, K, N)
    assert T().gemm_routes_load(f"{M + 8} {N} {K} PW 2 0 1 p8 1e+30 1e+30 0.02 0.01 129 1\n") == 1
    assert f"{M + 8} {N} {K} PW 2 0 1 p8" in T().gemm_routes()
    T().conv_pw_gemm_policy(1, 0)
    y, tot, done = fwd(gpu, x, w, M, N)
    assert rel_err(y, ref) < 1e-2
    assert f"{M} {N} {K} PW 2 0 1 " in T().gemm_routes()
