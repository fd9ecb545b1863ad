"""`-m gpu`: the paired correlation backward (vfi_correlation_backward_pair) and fused.corr_pair's autograd, bit for bit
against the C oracle (fmad=1) and against two vfi_correlation_backward calls.

Tiles are 64x4 pixels with a 4-pixel halo; blockIdx.z is role x image x channel group.  With all four gradients requested
the (B, C, H, W) shapes of SHAPES reach these (channel groups, channels per group):
    (1,1,1,1) (1,1);  (3,196,4,7) (98,2);  (1,5,4,64) (5,1);  (2,7,5,65) (7,1);  (1,3,9,130) (3,1);  (1,33,13,70) (33,1);
    (4,5,64,256) (2,3) -- channels split with a remainder;  (4,3,64,512) (1,3) -- one group, the double buffer runs all its steps
(groups = min(C, ceil(2048 / (tiles x B x roles))), then evened out: corr_backward_groups on the whole launch)."""
import ctypes
import itertools

import numpy as np
import pytest

from tests.test_gpu_parity import cpu, gpu, f32, torch_mod, cabi  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

PWC = (4, 1, 4, 1)          # pad, kernel, max displacement, stride2
SHAPES = [(1, 1, 1, 1), (3, 196, 4, 7), (1, 5, 4, 64), (2, 7, 5, 65), (1, 3, 9, 130), (1, 33, 13, 70), (4, 5, 64, 256), (4, 3, 64, 512)]


def _items(oracle, shape, cfg, seed, aliased=False):
    """two items of random data as numpy arrays: (a1, a2, ga, b1, b2, gb); aliased: (b1, b2) = (a2, a1)"""
    B, C, H, W = shape
    pad, k, md, s2 = cfg
    oc, oh, ow = oracle.correlation_out_dims(H, W, pad, k, md, 1, s2)
    rng = np.random.default_rng(seed)
    a1, a2, b1, b2 = (rng.standard_normal(shape).astype(f32) for _ in range(4))
    ga, gb = (rng.standard_normal((B, oc, oh, ow)).astype(f32) for _ in range(2))
    if aliased:
        b1, b2 = a2, a1
    return a1, a2, ga, b1, b2, gb


def _bits(t):
    return cpu(t).view(np.uint32)


def _check_pair(torch, cabi, oracle, host, cfg, aliased=False, with_oracle=True):
    pad, k, md, s2 = cfg
    a1, a2, ga, b1, b2, gb = (gpu(torch, x) for x in host)
    if aliased:
        b1, b2 = a2, a1                                     # the same tensor objects
    got = cabi.correlation_backward_pair(a1, a2, ga, b1, b2, gb, pad, k, md, 1, s2)
    single = cabi.correlation_backward(a1, a2, ga, pad, k, md, 1, s2) + cabi.correlation_backward(b1, b2, gb, pad, k, md, 1, s2)
    assert all(np.array_equal(_bits(g), _bits(s)) for g, s in zip(got, single))
    if with_oracle:
        ref = oracle.correlation_bwd(host[0], host[1], host[2], pad, k, md, 1, s2) + \
            oracle.correlation_bwd(host[3], host[4], host[5], pad, k, md, 1, s2)
        assert all(np.array_equal(cpu(g), r) for g, r in zip(got, ref))
    return got


@pytest.mark.parametrize("shape", SHAPES)
def test_tile_and_group_classes(torch_mod, cabi, oracle, shape):
    got = _check_pair(torch_mod, cabi, oracle, _items(oracle, shape, PWC, sum(shape)), PWC)
    assert any(np.abs(cpu(g)).max() > 0 for g in got)


def test_items_that_share_their_tensors(torch_mod, cabi, oracle):
    """(a1, a2, b1, b2) = (x, y, y, x), the same tensor objects: the top pyramid level of the two flow networks"""
    _check_pair(torch_mod, cabi, oracle, _items(oracle, (2, 7, 5, 65), PWC, 11, aliased=True), PWC, aliased=True)


def test_every_subset_of_outputs_through_the_c_abi(torch_mod, cabi, oracle):
    torch = torch_mod
    B, C, H, W = shape = (2, 7, 5, 65)
    host = _items(oracle, shape, PWC, 5)
    a1, a2, ga, b1, b2, gb = (gpu(torch, x) for x in host)
    single = cabi.correlation_backward(a1, a2, ga, 4, 1, 4, 1, 1) + cabi.correlation_backward(b1, b2, gb, 4, 1, 4, 1, 1)
    ref = oracle.correlation_bwd(*host[:3]) + oracle.correlation_bwd(*host[3:])
    assert all(np.array_equal(cpu(s), r) for s, r in zip(single, ref))
    fn = cabi.lib().vfi_correlation_backward_pair
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)  # noqa: E731
    subsets = [s for n in range(1, 5) for s in itertools.combinations(range(4), n)]
    assert len(subsets) == 15
    sentinel = float(np.float32(-7.25))
    for subset in subsets:
        outs = [torch.full(shape, sentinel, device="cuda:0") for _ in range(4)]       # (written in full: no sentinel survives)
        o = [outs[i] if i in subset else None for i in range(4)]
        # an item nothing is asked of passes NULL inputs and a NULL gradoutput
        ia = (a1, a2, ga) if (0 in subset or 1 in subset) else (None, None, None)
        ib = (b1, b2, gb) if (2 in subset or 3 in subset) else (None, None, None)
        err = fn(p(ia[0]), p(ia[1]), p(ia[2]), p(o[0]), p(o[1]), p(ib[0]), p(ib[1]), p(ib[2]), p(o[2]), p(o[3]),
                 B, C, H, W, 4, 1, 4, 1, 1, stream)
        assert err == 0, subset
        for i in range(4):
            if i in subset:
                assert np.array_equal(_bits(outs[i]), _bits(single[i])), (subset, i)
            else:
                assert (cpu(outs[i]) == sentinel).all(), (subset, i)


def test_wrapper_refuses_other_dtypes_and_returns_none_for_what_is_not_wanted(torch_mod, cabi, oracle):
    torch = torch_mod
    host = _items(oracle, (1, 3, 4, 5), PWC, 2)
    a1, a2, ga, b1, b2, gb = (gpu(torch, x) for x in host)
    with pytest.raises(RuntimeError, match="must be float32"):
        cabi.correlation_backward_pair(a1.half(), a2.half(), ga.half(), b1.half(), b2.half(), gb.half(), 4, 1, 4, 1, 1)
    with pytest.raises(RuntimeError, match="must be float32"):
        cabi.correlation_backward_pair(a1, a2, ga.double(), b1, b2, gb, 4, 1, 4, 1, 1)
    got = cabi.correlation_backward_pair(a1, a2, None, b1, b2, gb, 4, 1, 4, 1, 1, want=(True, True, False, True))
    assert got[0] is None and got[1] is None and got[2] is None
    assert np.array_equal(cpu(got[3]), oracle.correlation_bwd(*host[3:])[1])
    assert cabi.correlation_backward_pair(a1, a2, None, b1, b2, None, 4, 1, 4, 1, 1) == (None,) * 4


@pytest.mark.parametrize("cfg", [(3, 3, 4, 2), (2, 1, 4, 1), (4, 1, 2, 2)])
def test_other_configurations_take_the_single_launches(torch_mod, cabi, oracle, cfg):
    _check_pair(torch_mod, cabi, oracle, _items(oracle, (2, 5, 9, 20), cfg, sum(cfg)), cfg)


def test_grid_z_overflow_takes_the_single_launches(torch_mod, cabi, oracle):
    """four roles x 16400 images > 65535: one launch per gradient, the same bits"""
    _check_pair(torch_mod, cabi, oracle, _items(oracle, (16400, 1, 2, 3), PWC, 3), PWC)


def test_non_finite_values_on_and_next_to_the_border(torch_mod, cabi, oracle):
    """+-inf and NaN in gradoutput and in the inputs, on the frame border and one pixel inside it: the NaN positions and all
    other bits are the single calls' (compared as bit patterns)."""
    shape = (2, 7, 5, 65)
    host = [x.copy() for x in _items(oracle, shape, PWC, 21)]
    spots = [(0, 0), (0, 1), (1, 1), (4, 64), (3, 63), (4, 0), (2, 64), (1, 63)]       # (y, x): corners, edges and next to them
    vals = [np.inf, -np.inf, np.nan]
    for k, arr in enumerate(host):
        for j, (y, x) in enumerate(spots):
            if (j + k) % 2 == 0:
                arr[j % 2, (3 * j + k) % arr.shape[1], y, x] = vals[(j + k) % 3]
    got = _check_pair(torch_mod, cabi, oracle, host, PWC, with_oracle=False)
    assert all(np.isnan(cpu(g)).any() and np.isfinite(cpu(g)).any() for g in got)


def test_autograd_equals_two_single_correlation_graphs(torch_mod, cabi, oracle):
    torch = torch_mod
    from vfidkr_amd import fused
    shape = (2, 7, 5, 65)
    host = _items(oracle, shape, PWC, 31)
    wa, wb = gpu(torch, host[2]), gpu(torch, host[5])       # the loss: <out_a, wa> + <out_b, wb>

    def leaves(pattern):
        return [gpu(torch, host[i]).requires_grad_(r) for i, r in zip((0, 1, 3, 4), pattern)]

    def run(pattern, use_b=True):
        xs, ys = leaves(pattern), leaves(pattern)
        pa, pb = fused.corr_pair(*xs)
        sa = fused._Corr.apply(ys[0], ys[1])
        sb = fused._Corr.apply(ys[2], ys[3])
        assert np.array_equal(_bits(pa), _bits(sa)) and np.array_equal(_bits(pb), _bits(sb))
        assert pa.grad_fn is not None and pb.grad_fn is not None
        loss_p, loss_s = (pa * wa).sum(), (sa * wa).sum()
        if use_b:
            loss_p, loss_s = loss_p + (pb * wb).sum(), loss_s + (sb * wb).sum()
        loss_p.backward()
        loss_s.backward()
        return xs, ys

    xs, ys = run((True,) * 4)
    assert all(x.grad is not None and np.array_equal(_bits(x.grad), _bits(y.grad)) for x, y in zip(xs, ys))
    ref = oracle.correlation_bwd(*host[:3]) + oracle.correlation_bwd(*host[3:])
    assert all(np.array_equal(cpu(x.grad), r) for x, r in zip(xs, ref))
    # the loss uses only output a
    xs, ys = run((True,) * 4, use_b=False)
    assert xs[2].grad is None and xs[3].grad is None
    assert all(np.array_equal(_bits(x.grad), _bits(y.grad)) for x, y in zip(xs[:2], ys[:2]))
    # only the two c2 require grad
    xs, ys = run((False, True, False, True))
    assert xs[0].grad is None and xs[2].grad is None
    assert all(np.array_equal(_bits(xs[i].grad), _bits(ys[i].grad)) for i in (1, 3))
    # no_grad: today's path
    xs = leaves((True,) * 4)
    with torch.no_grad():
        outs = fused.corr_pair(*xs)
    plain = cabi.correlation_forward_pair(*[x.detach() for x in xs], 4, 1, 4, 1, 1)
    assert outs[0].grad_fn is None and outs[1].grad_fn is None
    assert all(np.array_equal(_bits(o), _bits(q)) for o, q in zip(outs, plain))


def test_pair_call_is_captured_and_replayed(torch_mod, cabi, oracle):
    """nothing is allocated by the entry: one call captured into a graph (one stream, a linear graph) and replayed twice"""
    torch = torch_mod
    B, C, H, W = shape = (2, 7, 5, 65)
    host = _items(oracle, shape, PWC, 41)
    a1, a2, ga, b1, b2, gb = (gpu(torch, x) for x in host)
    eager = cabi.correlation_backward_pair(a1, a2, ga, b1, b2, gb, 4, 1, 4, 1, 1)
    outs = [torch.zeros(shape, device="cuda:0") for _ in range(4)]
    fn = cabi.lib().vfi_correlation_backward_pair
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def call():
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert fn(p(a1), p(a2), p(ga), p(outs[0]), p(outs[1]), p(b1), p(b2), p(gb), p(outs[2]), p(outs[3]),
                  B, C, H, W, 4, 1, 4, 1, 1, stream) == 0

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            call()                                          # warm-up: the module is loaded before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        call()
    for _ in range(2):
        for o in outs:
            o.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert all(np.array_equal(_bits(o), _bits(e)) for o, e in zip(outs, eager))
