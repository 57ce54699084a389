"""Library graph capture (kern.graphed, gpsig_graph_begin / _end / _launch) at the state widths where the eager default is a route that does not
record: the wide route (csrc/wide_api.hip) and Kzx as a product of level features (csrc/sig_feat_api.hip).

The contract (include/gpsig_hip.h, graph section): after a warm-up under context option ``capture_routes`` a recording of the same call either
succeeds -- every replay bit-equal to an eager call under the option, and equal to the float64 oracle and to the default eager call (the other route) to
the tolerance tests/test_gpu_wide.py holds forward values to, 1e-10 of the largest entry -- or it was refused at the warm-up with a message that names
graph recording and the bound.  Never "a scratch buffer has to grow -- run the same calls once": the caller did.

Shapes: the smallest at which each route predicate of csrc/api.hip (the wide_auto_cols sites) flips; T inducing tensors, N sequences of L observations,
M levels.  Every case runs twice: through graphed(), and through ctx.graph() on a context that has served nothing else (scratch_bytes() == 0 before the
warm-up: torch hands side streams out from a pool, and a context that an earlier call left with large buffers would hide a warm-up on the wrong route).
Each prints its largest relative errors (profiles/graph_routes.txt)."""
import numpy as np
import pytest
import torch

from oracle import sigkern_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-10          # tests/test_gpu_wide.py: forward values against the oracle (no Matern-1/2 self-pair here)


def rel(a, b):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------
# id -> (kernel class, oracle base, d, M, T, N, N2, L, constructor keywords, [(method, tensors, call keywords, timing name of the default route)])
# timing name: what gpsig_timing_info reports when the default eager call ran -- the witness that it is the route that does not record
def _cases():
    a = lambda inc: ("K_tens_vs_seq", "ZX", dict(increments=inc), "wide_tvs")        # noqa: E731
    return {
        "a_rbf_kzx_d9": ("SignatureRBF", "rbf", 9, 3, 5, 12, 0, 10, {}, [a(True), a(False)]),
        "b_rbf_kzx_few_d6": ("SignatureRBF", "rbf", 6, 3, 5, 12, 0, 10, {}, [a(True)]),
        "c_rbf_kzz_d13": ("SignatureRBF", "rbf", 13, 3, 5, 0, 0, 0, {}, [("K_tens", "Z", dict(increments=True), "wide_tens"), ("K_tens", "Z", dict(increments=False), "wide_tens")]),
        # K reroute: more than 16 columns and pairs_hint >= 4096 -- 90 * (90 / 2 + 1) = 4,140 for the symmetric Gram, 90 * 64 = 5,760 for the cross one
        "d_rbf_k_d17": ("SignatureRBF", "rbf", 17, 3, 0, 90, 64, 6, {}, [("K", "X", {}, "wide_lattice"), ("K", "XY", {}, "wide_lattice")]),
        "e_rbf_k_d33": ("SignatureRBF", "rbf", 33, 3, 0, 10, 0, 6, {}, [("K", "X", {}, "wide_lattice")]),
        "e_rbf_kdiag_d33": ("SignatureRBF", "rbf", 33, 3, 0, 10, 0, 6, dict(normalization=False), [("Kdiag", "X", {}, "wide_lattice")]),
        "f_matern32_kzx_d9": ("SignatureMatern32", "matern32", 9, 3, 5, 12, 0, 10, {}, [a(True), a(False)]),
        "g_rbf_order2_lag1_d5": ("SignatureRBF", "rbf", 5, 3, 5, 12, 0, 10, dict(order=2, num_lags=1), [a(True)]),
        # the product wins tvs_features_plan's time model from about 5,700 sequences on at this shape (tile: 40 us + T N L lt / 4e12 = 124 us at 8,192; product: 100 us)
        "h_linear_kzx_features": ("SignatureLinear", "linear", 3, 4, 128, 8192, 0, 32, {}, [("K_tens_vs_seq", "ZX", dict(increments=False), "tvs_features")]),
        "i_linear_d33": ("SignatureLinear", "linear", 33, 2, 5, 10, 0, 6, {}, [("K", "X", {}, "wide_lattice"), ("K_tens_vs_seq", "ZX", dict(increments=False), "wide_tvs")]),
    }


CASES = _cases()
ORACLE_ROWS = 32           # case (h): the oracle on the first sequences only (Kzx is normalised sequence by sequence: its columns are independent)


class Case:
    """The kernel object, its oracle, and for every call of the case the tensors (two sets of contents) and the oracle's value on the second set --
    computed once, shared by the tests of the case, never written."""

    def __init__(self, name):
        from gpsig_amd import kernels
        cls, base, d, M, T, N, N2, L, kw, calls = CASES[name]
        rng = np.random.default_rng(sum(map(ord, name)))
        lags = int(kw.get("num_lags") or 0)
        de, lt = d * (lags + 1), M * (M + 1) // 2
        ls, var = rng.uniform(0.8, 1.6, d), rng.uniform(0.5, 1.5, M + 1)
        self.name, self.d = name, d
        self.kern = getattr(kernels, cls)(max(L, 1) * d, d, M, lengthscales=ls, variances=var, **kw)
        self.oracle = O.SignatureKernelOracle(max(L, 1) * d, d, M, base=base, lengthscales=ls, variances=var, **kw)
        s = 1.0 / np.sqrt(d)                                     # distances of order one whatever the width
        seq = lambda n: np.cumsum(rng.standard_normal((n, L, d)) * 0.5 * s, axis=1).reshape(n, L * d)      # noqa: E731
        self.calls = []
        for method, what, ckw, route in calls:
            shapes = {"Z": (lt, T, 2, de) if ckw.get("increments") else (lt, T, de)}
            host = [[(rng.standard_normal(shapes["Z"]) * s if w == "Z" else seq(N if w == "X" else N2)) for w in what] for _ in range(2)]
            ref = [h[:ORACLE_ROWS] if (w == "X" and method == "K_tens_vs_seq") else h for w, h in zip(what, host[1])]
            want = getattr(self.oracle, method)(*ref, **ckw)
            want.setflags(write=False)
            self.calls.append((method, ckw, route, host, want))

    def tensors(self, host):
        return [torch.tensor(h, device=DEV) for h in host]


_built = {}


def case(name):
    if name not in _built:
        _built[name] = Case(name)
    return _built[name]


def call_ids():
    return [(n, k) for n, c in CASES.items() for k in range(len(c[9]))]


def under_option(ctx, fn, name="capture_routes", value=1, default=0):
    try:
        ctx.set_option(name, value)
        return fn()
    finally:
        ctx.set_option(name, default)


def current_ctx():
    from gpsig_amd import _lib
    return _lib.context(0, torch.cuda.current_stream(DEV).cuda_stream)


def own_context():
    """A stream whose context has served nothing: torch's side streams come from a pool, so look for one no context exists for; if every pooled stream
    has one, drop a context that no recording holds."""
    from gpsig_amd import _lib
    streams = [torch.cuda.Stream(DEV) for _ in range(40)]
    s = next((s for s in streams if (0, s.cuda_stream) not in _lib._contexts), None)
    if s is None:
        s = next(s for s in streams if (0, s.cuda_stream) not in _lib._holders)
        s.synchronize()
        _lib._contexts.pop((0, s.cuda_stream)).close()
    ctx = _lib.context(0, s.cuda_stream)
    ctx.set_pointer_mode(_lib.PTR_DEVICE)
    _lib.hold(0, s.cuda_stream)
    return s, ctx


def check_values(c, tag, method, replay, want, default):
    """checks 3 .. 5 of a replay on the second contents; prints the figures before it asserts"""
    got = replay[:, :ORACLE_ROWS] if method == "K_tens_vs_seq" and replay.shape[1] > want.shape[1] else replay
    e_or, e_def = rel(got, want), rel(replay, default)
    print("graph_routes %-24s %-14s %-10s vs oracle %.3e   vs default eager route %.3e" % (c.name, method, tag, e_or, e_def))
    assert not torch.equal(replay, torch.zeros_like(replay))
    assert e_or < TOL, (c.name, method, tag, e_or)
    assert e_def < TOL, (c.name, method, tag, e_def)


# ---- every case through graphed() ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", call_ids())
def test_graphed_records_on_the_route_it_replays(name, k):
    c = case(name)
    method, ckw, route, host, want = c.calls[k]
    tens = c.tensors(host[0])
    fn = lambda: getattr(c.kern, method)(*tens, **ckw)          # noqa: E731
    g = c.kern.graphed(method, *tens, **ckw)                     # (1) records
    assert not c.kern._graph_recording
    ctx = current_ctx()
    assert torch.equal(g.out, under_option(ctx, fn))             # recorded on the first contents
    for t, h in zip(tens, host[1]):
        t.copy_(torch.tensor(h, device=DEV))
    got = g.replay().clone()
    assert torch.equal(got, under_option(ctx, fn)), (name, method)         # (2) the route the recording took
    ctx.timing_reset()
    default = fn()
    if route is not None:                                        # the default eager call is the other route: the one that does not record
        assert route in str(ctx.timing_info()[0]), (name, method, ctx.timing_info())
    check_values(c, "graphed()", method, got, want, default)
    # the side stream's context is back on the default routes: bit-equal to a plain context's answer
    with torch.cuda.stream(g.stream):
        again = fn()
    g.stream.synchronize()
    assert torch.equal(again, default)
    g.close()


# ---- ... and through ctx.graph() on a context that has served nothing else ---------------------------------------------------------------------
@pytest.mark.parametrize("name,k", call_ids())
def test_fresh_context_warm_up_sizes_the_recorded_route(name, k):
    from gpsig_amd import _lib
    c = case(name)
    method, ckw, route, host, want = c.calls[k]
    tens = c.tensors(host[0])
    fn = lambda: getattr(c.kern, method)(*tens, **ckw)          # noqa: E731
    torch.cuda.synchronize()
    s, ctx = own_context()
    graph = None
    try:
        with torch.cuda.stream(s):
            assert ctx.scratch_bytes() == 0
            under_option(ctx, fn)                                # the documented warm-up
            with ctx.graph() as graph:                           # (1) records: no buffer has to grow
                out = fn()
            s.synchronize()
            for t, h in zip(tens, host[1]):
                t.copy_(torch.tensor(h, device=DEV))
            out.zero_()
            graph.launch()
            s.synchronize()
            got = out.clone()
            assert torch.equal(got, under_option(ctx, fn)), (name, method)     # (2)
            s.synchronize()
        default = fn()                                           # the current stream's context: default routes
        check_values(c, "ctx.graph()", method, got, want, default)
    finally:
        s.synchronize()
        if graph is not None:
            graph.destroy()
        _lib.release(0, s.cuda_stream)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
def _refusal_cases():
    from gpsig_amd import kernels
    import test_gpu_wide_spectral as WS
    rng = np.random.default_rng(65)
    M, T, N, L = 3, 5, 6, 5
    lt = M * (M + 1) // 2
    d = 65
    rbf = kernels.SignatureRBF(L * d, d, M, lengthscales=np.sqrt(d))
    X = torch.tensor(np.cumsum(rng.standard_normal((N, L, d)) * 0.3, axis=1).reshape(N, -1), device=DEV)
    Z = torch.tensor(rng.standard_normal((lt, T, d)), device=DEV)
    ds = 33
    spec, _ = WS.make("gauss", 2, L, ds, 2)                      # exact SignatureSpectral, spectral_wide = True
    Xs = torch.tensor(np.cumsum(rng.standard_normal((N, L, ds)) * 0.3, axis=1).reshape(N, -1), device=DEV)
    return [(rbf, "K_tens_vs_seq", (Z, X), "64 columns"), (rbf, "K", (X,), "64 columns"), (spec, "K", (Xs,), "32 columns")]


@pytest.mark.parametrize("k", range(3))
def test_shapes_with_no_route_but_the_wide_one_are_refused_at_the_warm_up(k):
    from gpsig_amd import _lib
    kern, method, tens, bound = _refusal_cases()[k]
    before = getattr(kern, method)(*tens).clone()
    contexts = set(_lib._contexts)
    with pytest.raises(NotImplementedError) as ei:
        kern.graphed(method, *tens)
    msg = str(ei.value)
    assert "graph recording" in msg and "wide route only, which does not record" in msg and bound in msg, msg
    assert "scratch buffer" not in msg and "run the same calls once" not in msg
    assert not kern._graph_recording
    assert set(_lib._contexts) <= contexts                       # the side stream's context was given back
    assert torch.equal(getattr(kern, method)(*tens), before)
    # the C ABI's own refusal, inside a capture on a context that was warmed up WITHOUT the option (what a caller unaware of it does): the same words
    s, ctx = own_context()
    try:
        with torch.cuda.stream(s):
            want = getattr(kern, method)(*tens).clone()
            with pytest.raises(NotImplementedError, match="graph recording.*which does not record"):
                with ctx.graph():
                    getattr(kern, method)(*tens)
            assert torch.equal(getattr(kern, method)(*tens), want)           # no capture left open: the context works as before
            s.synchronize()
    finally:
        _lib.release(0, s.cuda_stream)


# ---- the option itself ---------------------------------------------------------------------------------------------------------------------------
def test_option_skips_only_the_wide_route_at_nine_columns():
    """With the option set and no capture, case (a) is bit-equal to eager under wide = 0: both skip only the wide route there."""
    c = case("a_rbf_kzx_d9")
    ctx = current_ctx()
    for method, ckw, route, host, want in c.calls:
        tens = c.tensors(host[1])
        fn = lambda: getattr(c.kern, method)(*tens, **ckw)      # noqa: E731
        ctx.timing_reset()
        as_captured = under_option(ctx, fn)
        assert route not in str(ctx.timing_info()[0])
        assert torch.equal(as_captured, under_option(ctx, fn, "wide", 0, -1))
        ctx.timing_reset()
        fn()
        assert route in str(ctx.timing_info()[0])                # ... and it is back: the default route again


class _Shim:
    """`target` with some attributes replaced"""

    def __init__(self, target, **over):
        self._target, self._over = target, over

    def __getattr__(self, name):
        return self._over[name] if name in self._over else getattr(self._target, name)


def test_option_is_restored_when_graphed_raises(monkeypatch):
    """graphed() on a side stream whose context another recording holds (torch's pool hands streams out again): after a refusal the option is back
    at 0 on that context -- it takes the default route again, bit-equal to a plain context's answer."""
    from gpsig_amd import _lib
    c = case("a_rbf_kzx_d9")
    method, ckw, route, host, want = c.calls[0]
    tens = c.tensors(host[1])
    fn = lambda: getattr(c.kern, method)(*tens, **ckw)          # noqa: E731
    plain = fn()
    before_stream = torch.cuda.current_stream(DEV).cuda_stream
    kern, rmethod, rtens, _ = _refusal_cases()[0]
    s, ctx = own_context()                                       # (holds the context, as a live recording would)
    try:
        # graphed() asks torch.cuda.Stream for its side stream: the kernels module alone sees one that hands out `s` (torch itself must not: its own
        # stream bookkeeping constructs torch.cuda.Stream objects)
        from gpsig_amd import kernels
        monkeypatch.setattr(kernels, "torch", _Shim(torch, cuda=_Shim(torch.cuda, Stream=lambda *a, **kw: s)))
        with pytest.raises(NotImplementedError, match="graph recording"):
            kern.graphed(rmethod, *rtens)
        monkeypatch.undo()
        assert _lib._contexts.get((0, s.cuda_stream)) is ctx and not kern._graph_recording
        with torch.cuda.stream(s):
            ctx.timing_reset()
            again = fn()
            assert route in str(ctx.timing_info()[0])
            s.synchronize()
        assert torch.equal(again, plain)
        assert torch.cuda.current_stream(DEV).cuda_stream == before_stream
    finally:
        monkeypatch.undo()
        _lib.release(0, s.cuda_stream)
