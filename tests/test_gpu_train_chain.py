"""GPU suite (`-m gpu`): one miniature DAIN / DAIN_slowmotion training step made only of the library's trainable entries
(tests/train_chain.py), run as ONE autograd graph and checked against an independent wiring of the same step, against the
CPU oracle and against a float64 statement of the graph.

Wirings: A the fused entries, B the compositions they are documented to equal, O the CPU oracle (float32), R float64 torch
with O's decisions.  A mismatch is reported at the most downstream tensor first, which names the Function at fault.

Which gradients of A and B must agree bit for bit, and which only within the bound against R:
  * `dain` with only pixel losses in total: everything.  Each gradient is a single term or a two-term sum, and a two-term
    float sum does not depend on its order.
  * `slowmo` / `slowmo_bf16`, BIT_EQUAL: the out_t and buffer gradients (the same torch ops on the same bits), the taps (a
    projected flow's gradient from the synthesis stage alone: kernel term + passed-through slice), the projected flows
    (tap + the loss's term), the context and depth gradients and flow_q's (one call, or a sum in list order, over
    bit-equal incoming gradients), the cost volumes and the features (one or two terms).
  * `slowmo`, WITHIN_BOUND only: frames and filters (per time offset a kernel term and a passed-through slice: up to six
    terms, whose order autograd does not promise) and the coarse flow `flo` (four terms: flow_q of both directions and both
    warps).
  * cur_t: in A `cur_output` is an output of its own beside the buffer, so its gradient lacks the term through the buffer's
    channels 0-2 that A's Function adds inside; against R and B it is compared as grad(cur_t) + grad(buf_t)[:, 0:3].
"""
import pytest

from tests import train_chain as tc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WITHIN_BOUND = ("ref0", "ref2", "filt0", "filt1", "flo")


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("`-m gpu` tests need a GPU: torch.cuda.is_available() is False")
    return torch


@pytest.fixture(scope="module")
def cabi(torch_mod):
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import cabi as c
    assert "gfx950" in c.version()
    return c


@pytest.fixture(scope="module")
def fused(cabi):
    from vfidkr_amd import fused as f
    return f


def run(torch, fused, name, wiring="A", **kw):
    ops = tc.FusedOps(torch, fused, wiring, bf16=tc.CONFIGS[name]["bf16"])
    L, T, total, G = tc.run(torch, ops, name, device=DEV, **kw)
    torch.cuda.synchronize()
    return L, T, total, G


@pytest.fixture(scope="module")
def full(torch_mod, fused):
    """(leaves, tensors, total, gradients) of a whole step, every leaf requiring grad and every loss in total: computed
    once per (configuration, wiring) and shared; read-only"""
    cache = {}

    def get(name, wiring="A"):
        if (name, wiring) not in cache:
            cache[name, wiring] = run(torch_mod, fused, name, wiring)
        return cache[name, wiring]
    return get


def with_whole_cur(G, wiring):
    """the gradients with cur_t's made comparable across wirings (module docstring)"""
    if not wiring.startswith("A"):
        return G
    G = dict(G)
    for k in list(G):
        if k.startswith("cur") and G[k] is not None:
            b = G["buf" + k[3:]]
            G[k] = G[k] if b is None else G[k] + b[:, 0:3].to(G[k].dtype)
    return G


def assert_same_bits(torch, got, want, what, names=None):
    k = tc.first_mismatch(torch, got, want, names)
    assert k is None, "%s: %s differs (the most downstream tensor that does)" % (what, k)


def assert_inside(got, ref, key, what, names=None):
    bad = tc.outside_bound(got, ref, key, names)
    assert not bad, "%s: outside the bound, the most downstream first: %s" % (
        what, ", ".join("%s %.3g > %.3g" % b for b in bad))


# ------------------------------------------------------------------ 1. forward A = O

@pytest.mark.parametrize("name", ["dain", "slowmo"])
def test_forward_equals_the_oracle_bit_for_bit(torch_mod, full, name):
    """every intermediate up to and including the rectify buffers: the GPU and the oracle take the same decisions.  out_t
    and the loss values sit behind a reduction: within the bound."""
    torch = torch_mod
    TO, _, TR, _, _ = tc.oracle_and_reference(name)
    for wiring in ("A", "B"):
        T = full(name, wiring)[1]
        for k in T:                                         # (forward: the most upstream first)
            if k.startswith(("out", "loss_")):
                e, b = tc.rel_err(T[k], TR[k]), tc.bound(name, "value_" + k)
                assert e <= b, "%s %s: %s is %.3g from R, bound %.3g" % (name, wiring, k, e, b)
            else:
                assert tc.same_bits(torch, T[k].detach().cpu(), TO[k].detach()), "%s %s: forward %s differs from the oracle's" % (name, wiring, k)


# ------------------------------------------------------------------ 2. gradients against R

@pytest.mark.parametrize("wiring", ["A", "A_pair", "B"])
@pytest.mark.parametrize("name", ["dain", "slowmo"])
def test_gradients_against_the_float64_reference(full, name, wiring):
    """every leaf and intermediate, no element excluded"""
    GR = tc.oracle_and_reference(name)[3]
    G = with_whole_cur(full(name, wiring)[3], wiring)
    assert all(G[k] is not None for k in G)
    assert set(tc.LEAVES) & set(GR) <= set(G)
    assert_inside(G, GR, name, "%s %s" % (name, wiring))


# ------------------------------------------------------------------ 3. A = B

def test_dain_pixel_losses_fused_equals_unfused_everywhere(torch_mod, fused):
    torch = torch_mod
    terms = tuple(tc.pixel_names(tc.CONFIGS["dain"]))
    GB = run(torch, fused, "dain", "B", loss_terms=terms)[3]
    for wiring in ("A", "A_pair"):
        GA = with_whole_cur(run(torch, fused, "dain", wiring, loss_terms=terms)[3], wiring)
        assert all(GA[k] is not None for k in tc.LEAVES if k in GA)
        assert_same_bits(torch, GA, GB, "dain, pixel losses, %s against B" % wiring)


@pytest.mark.parametrize("name", ["slowmo", "slowmo_bf16"])
def test_slowmo_fused_equals_unfused(torch_mod, fused, full, name):
    torch = torch_mod
    GA, GB = with_whole_cur(full(name, "A")[3], "A"), full(name, "B")[3]
    exact = [k for k in GA if k in GB and k not in WITHIN_BOUND and not k.startswith("cur")]
    assert {"tap0_0", "tap1_2", "proj0_1", "ctx0", "ctx2", "depth0", "depth1", "flow_q0", "flow_q1", "f1", "f2"} <= set(exact)
    assert_same_bits(torch, GA, GB, "%s: A against B" % name, exact)
    if name == "slowmo":
        GR = tc.oracle_and_reference(name)[3]
        for G, w in ((GA, "A"), (GB, "B")):
            assert_inside(G, GR, name, "%s %s" % (name, w), WITHIN_BOUND + tuple(k for k in GA if k.startswith("cur")))
    else:
        # bfloat16: no float64 bound is asked; the order-dependent sums of A and B agree within the float32 configuration's
        # bound, and a second run gives the first run's bits
        for k in WITHIN_BOUND:                              # (the same float32 sums as in `slowmo`: its bound, here between A and B)
            assert tc.rel_err(GA[k], GB[k]) <= tc.bound("slowmo", k), k
        again = with_whole_cur(run(torch, fused, name, "A")[3], "A")
        assert_same_bits(torch, again, GA, "%s: second run" % name)


# ------------------------------------------------------------------ 4. requires-grad subsets

@pytest.mark.parametrize("subset", ["flows", "filters", "contexts", "depths", "frames", "all but contexts", "depth1"])
def test_requires_grad_subsets(torch_mod, fused, full, subset):
    """only part of the model trains: each requested gradient has the full run's bits, nothing else gets one.  `depth1`
    alone makes the two directions' projected flows differ in requires_grad."""
    torch = torch_mod
    want = tc.GROUPS.get(subset, (subset,))
    L, T, total, G = run(torch, fused, "slowmo", "A", requires=want)
    GF = full("slowmo", "A")[3]
    for leaf in tc.LEAVES:
        if leaf in want:
            assert tc.same_bits(torch, G[leaf], GF[leaf]), "%s: grad %s differs from the full run's" % (subset, leaf)
        else:
            assert G[leaf] is None, leaf
    inner = [k for k in G if k not in tc.LEAVES and G[k] is not None and not k.startswith("cur")]
    assert_same_bits(torch, G, GF, "subset %s" % subset, inner)


# ------------------------------------------------------------------ 5. loss subsets

@pytest.mark.parametrize("wiring", ["A", "B"])
@pytest.mark.parametrize("subset", sorted(tc.LOSS_SUBSETS))
def test_loss_subsets(torch_mod, fused, subset, wiring):
    """total made of part of the losses: the other outputs are absent items.  Each gradient matches O within the bound;
    what the loss cannot reach has no gradient at all (None, not zeros)."""
    torch = torch_mod
    terms = tc.LOSS_SUBSETS[subset]
    _, GO, _, GR, _ = tc.oracle_and_reference("slowmo", terms)
    G = with_whole_cur(run(torch, fused, "slowmo", wiring, loss_terms=terms)[3], wiring)
    key = "slowmo/" + subset
    for k in G:
        if k not in GO:
            continue
        assert (G[k] is None) == (GO[k] is None), "%s %s: %s is %s" % (subset, wiring, k, "None" if G[k] is None else "a tensor")
    if subset == "flow terms":
        assert all(G[k] is None for k in ("ref0", "ref2", "filt0", "filt1", "ctx0", "ctx2", "buf1", "cur1"))
    if subset == "cur only":
        assert G["buf0"] is None and G["ctx0"] is None and G["cur0"] is not None and G["ref0"] is not None
    if subset == "one pixel":
        assert G["buf0"] is None and G["buf2"] is None and G["tap0_0"] is None and G["buf1"] is not None
    bad = []
    for k in G:
        if k in GO and GO[k] is not None:
            e = tc.rel_err(G[k], GO[k]) * float(GO[k].abs().max()) / float(GR[k].abs().max())
            if not e <= tc.bound(key, k):
                bad.append("%s %.3g > %.3g" % (k, e, tc.bound(key, k)))
    assert not bad, "%s %s: outside the bound against O, the most downstream first: %s" % (subset, wiring, ", ".join(bad))


# ------------------------------------------------------------------ 6. repetition

def test_the_same_step_twice(torch_mod, fused, full):
    torch = torch_mod
    for name in ("dain", "slowmo"):
        first = full(name, "A")
        _, T, _, G = run(torch, fused, name, "A")
        assert_same_bits(torch, {k: v.detach() for k, v in T.items()}, {k: v.detach() for k, v in first[1].items()}, name + ": forward")
        assert_same_bits(torch, G, first[3], name + ": second step")


def test_two_backward_passes_through_one_graph(torch_mod, fused, full):
    """backward(retain_graph=True) twice, into fresh .grad: part_loss's `used` set and every workspace start over"""
    torch = torch_mod
    ops = tc.FusedOps(torch, fused, "A")
    L = tc.leaves(torch, "slowmo", DEV)
    T, total = tc.step(torch, ops, L, "slowmo")
    for turn in range(2):
        for v in list(L.values()) + list(T.values()):
            v.grad = None
        total.backward(retain_graph=True)
        torch.cuda.synchronize()
        assert_same_bits(torch, tc.gradients(T, L), full("slowmo", "A")[3], "backward pass %d" % turn)
    # ... and a pass that uses other losses than the one before it, through the same graph
    for v in list(L.values()) + list(T.values()):
        v.grad = None
    T["loss_out1"].backward(retain_graph=True)
    one = {k: (None if v is None else v.clone()) for k, v in tc.gradients(T, L).items()}
    for v in list(L.values()) + list(T.values()):
        v.grad = None
    (T["loss_offset"] * tc.OFFSET_W + T["loss_sym"] * tc.SYM_W).backward()
    torch.cuda.synchronize()
    G = tc.gradients(T, L)
    assert G["ref0"] is None and G["ctx0"] is None and G["depth0"] is not None and one["ref0"] is not None
    want = run(torch, fused, "slowmo", "A", loss_terms=tc.LOSS_SUBSETS["flow terms"])[3]
    assert_same_bits(torch, G, want, "flow terms after one pixel loss")


def test_frame_sizes_in_turn(torch_mod, fused, full):
    """36 x 80, 68 x 140, 36 x 80, 68 x 140: stale or regrown workspaces would change a bit"""
    torch = torch_mod
    small = full("slowmo", "A")[3]
    big = run(torch, fused, "slowmo_big", "A")[3]
    assert all(big[k] is not None for k in big)
    assert_same_bits(torch, run(torch, fused, "slowmo", "A")[3], small, "36 x 80 after 68 x 140")
    assert_same_bits(torch, run(torch, fused, "slowmo_big", "A")[3], big, "68 x 140 after 36 x 80")
    bigB = run(torch, fused, "slowmo_big", "B")[3]
    exact = [k for k in big if k in bigB and k not in WITHIN_BOUND and not k.startswith("cur")]
    assert_same_bits(torch, big, bigB, "68 x 140: A against B", exact)


def test_side_stream_then_default_stream(torch_mod, fused, full):
    torch = torch_mod
    want = full("slowmo", "A")[3]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        G = run(torch, fused, "slowmo", "A")[3]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert_same_bits(torch, G, want, "on a side stream")
    assert_same_bits(torch, run(torch, fused, "slowmo", "A")[3], want, "on the default stream afterwards")


# ------------------------------------------------------------------ 7. checkpoint

@pytest.mark.parametrize("wiring", ["A", "B"])
def test_checkpoint_around_projection_and_synthesis(torch_mod, fused, full, wiring):
    """torch.utils.checkpoint(use_reentrant=False) around stages 2-3: the Functions run their forward a second time inside
    the backward pass, and their backward may unpack its saved tensors only once; same bits"""
    torch = torch_mod
    _, T, _, G = run(torch, fused, "slowmo", wiring, checkpoint=True)
    want = full("slowmo", wiring)[3]
    assert_same_bits(torch, G, want, "checkpointed " + wiring, [k for k in G if k in tc.LEAVES or k.startswith(("flow_q", "cost", "out"))])


# ------------------------------------------------------------------ 8. inference

@pytest.mark.parametrize("name", ["dain", "slowmo", "slowmo_bf16"])
def test_inference_forward_is_the_training_forward(torch_mod, fused, full, name):
    torch = torch_mod
    with torch.no_grad():
        _, T, total, _ = run(torch, fused, name, "A", backward=False)
    assert total is None and all(v.grad_fn is None for v in T.values())
    train = full(name, "A")[1]
    assert_same_bits(torch, T, {k: v.detach() for k, v in train.items()}, name + ": inference forward")
    buf, cur = T["buf0"], T["cur0"]
    if name == "slowmo_bf16":                               # (cur_output stays float32 and a tensor of its own)
        assert cur.dtype == torch.float32 and buf.dtype == torch.bfloat16
    else:                                                   # the view form
        assert cur.data_ptr() == buf.data_ptr() and cur.stride() == buf[:, 0:3].stride() and cur.shape == buf[:, 0:3].shape
    # no leaf requires grad, grad mode on: the same plain launches
    _, T2, total2, _ = run(torch, fused, name, "A", requires=(), backward=False)
    assert total2 is None
    assert_same_bits(torch, T2, T, name + ": nothing requires grad")


# ------------------------------------------------------------------ 9. a captured step

def test_a_captured_step_replays_the_eager_gradients(torch_mod, fused, full):
    """forward and backward of `dain` in one torch.cuda.graph on a side stream (a linear graph), after a warm-up there
    that lets every workspace reach its size; three replays, each the eager run's bits.
    This test found that the fixed-point accumulator's per-call hipMemsetAsync did not hold as a memset node from the
    second replay on (the gradients of ref0, ref2 and f2 came out scaled by a stale header); gradacc_reserve zero-fills with
    a kernel since."""
    torch = torch_mod
    want = full("dain", "A")[3]
    ops = tc.FusedOps(torch, fused, "A")
    L = tc.leaves(torch, "dain", DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):                                  # warm-up on the capture stream
            T, total = tc.step(torch, ops, L, "dain")
            total.backward()
            for v in L.values():
                v.grad = None
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    del T, total
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        T, total = tc.step(torch, ops, L, "dain")
        total.backward()
    G = tc.gradients(T, L)
    for turn in range(3):
        for g in G.values():
            g.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert_same_bits(torch, G, want, "replay %d" % turn)
    del graph
