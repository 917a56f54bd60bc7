"""ctypes binding of the C++ host side (svinet_amd/host/capi.cc).

Gives Python the PRODUCT's own graph reader, held-out sampler, gamma/lambda
initialisation and training-link list (the reference's Network::read and
LinkSampling constructor, src/network.cc:10-116, src/linksampling.cc:5-155),
so that bench.py and the tests feed the device C ABI with product-made inputs.
"""
import ctypes as C
import os

import numpy as np

from . import _svils

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libsvinet_host.so")
ETA_TYPES = {"uniform": 0, "fromdata": 1, "sparse": 2, "dense": 3}


class Options(C.Structure):
    _fields_ = [("n", C.c_uint32), ("k", C.c_uint32), ("seed", C.c_double),
                ("heldout_ratio", C.c_double), ("link_thresh", C.c_double),
                ("lt_min_deg", C.c_uint32), ("eta_type", C.c_int32), ("accuracy", C.c_int32), ("defer_gamma", C.c_int32),
                ("batch_device", C.c_int32), ("device", C.c_int32), ("sampled", C.c_int32), ("nodelay", C.c_int32),
                ("tau0", C.c_double), ("kappa", C.c_double), ("nodetau0", C.c_double), ("nodekappa", C.c_double),
                ("inf_epsilon", C.c_double), ("logl", C.c_int32), ("sparse_graph", C.c_int32)]


_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OSError("%s not found: run `python -m svinet_amd.build`" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, u32, u64, dbl = C.c_void_p, C.c_uint32, C.c_uint64, C.c_double
    P = C.POINTER
    L.svih_options_default.argtypes = [P(Options), u32, u32]
    L.svih_options_default.restype = None
    L.svih_setup_from_file.argtypes = [C.c_char_p, P(Options)]
    L.svih_setup_from_file.restype = vp
    L.svih_setup_from_pairs.argtypes = [vp, u64, P(Options)]
    L.svih_setup_from_pairs.restype = vp
    L.svih_setup_free.argtypes = [vp]
    L.svih_setup_free.restype = None
    for name, res in (("n", u32), ("k", u32), ("ones", u32), ("singles", u32),
                      ("total_pairs", dbl), ("ones_prob", dbl), ("eta0", dbl), ("eta1", dbl),
                      ("seq2id", P(u32)), ("gamma", P(dbl)), ("lambda", P(dbl)),
                      ("nvalidation", u64), ("validation_sorted", P(u32)),
                      ("validation_accept", P(u32)), ("nlinks", u64), ("links", P(u32)),
                      ("edges", P(u32))):
        f = getattr(L, "svih_" + name)
        f.argtypes = [vp]
        f.restype = res
    L.svih_init_links.argtypes = [vp, vp]
    L.svih_init_links.restype = u64
    L.svih_init_offset.argtypes = [vp]
    L.svih_init_offset.restype = u64
    L.svih_init_streams.argtypes = [vp, u64, u64, vp]
    L.svih_init_streams.restype = C.c_int
    L.svih_deg.argtypes = [vp, u32]
    L.svih_deg.restype = u32
    L.svih_findk_from_file.argtypes = [C.c_char_p, P(Options), C.c_int]
    L.svih_findk_from_file.restype = vp
    L.svih_findk_from_pairs.argtypes = [vp, u64, P(Options), C.c_int]
    L.svih_findk_from_pairs.restype = vp
    for name, res in (("free", None), ("step", C.c_int), ("n", u32), ("iter", u32), ("unlikely", u32), ("npad", u32),
                      ("pad_seconds", dbl), ("training_ll", dbl), ("nheldout", u64), ("heldout", P(u32)), ("seq2id", P(u32))):
        f = getattr(L, "svih_findk_" + name)
        f.argtypes = [vp]
        f.restype = res
    L.svih_findk_row.argtypes = [vp, vp]
    L.svih_findk_row.restype = None
    L.svih_findk_state.argtypes = [vp, vp, vp, vp]
    L.svih_findk_state.restype = None
    L.svih_findk_timing.argtypes = [vp, vp]
    L.svih_findk_timing.restype = C.c_int
    L.svih_ppc_philox.argtypes = [vp, u64, vp, vp]
    L.svih_ppc_philox.restype = None
    L.svih_ppc_dirichlet.argtypes = [vp, u32, u32, u32, u32, vp]
    L.svih_ppc_dirichlet.restype = None
    L.svih_ppc_beta.argtypes = [vp, u32, u32, u32, vp]
    L.svih_ppc_beta.restype = None
    _lib = L
    return L


def _arr(ptr, shape, dtype):
    n = int(np.prod(shape))
    if n == 0:
        return np.zeros(shape, dtype=dtype)
    return np.ctypeslib.as_array(ptr, shape=(n,)).view(dtype).reshape(shape).copy()


class Setup:
    """Host-side state of `LinkSampling ls(env, network)` before infer()."""

    def __init__(self, path=None, n=0, k=0, pairs=None, seed=0, heldout_ratio=0.01,
                 link_thresh=0.5, lt_min_deg=0, eta_type="uniform", accuracy=False, host_gamma=True):
        """host_gamma=False: init_gamma2 is NOT drawn on the host (2.9 s and a 4.1 GB array at n = 1e6, k = 512); engines get their
        gamma from svils_init_gamma (device_init), bit-identical to the host path"""
        L = load()
        o = Options()
        L.svih_options_default(C.byref(o), n, k)
        o.seed = seed
        o.heldout_ratio = heldout_ratio
        o.link_thresh = link_thresh
        o.lt_min_deg = lt_min_deg
        o.eta_type = ETA_TYPES[eta_type]
        o.accuracy = int(accuracy)
        o.defer_gamma = 0 if host_gamma else 1
        self.host_gamma = bool(host_gamma)
        if pairs is not None:
            pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
            self._h = L.svih_setup_from_pairs(pairs.ctypes.data, pairs.shape[0], C.byref(o))
        else:
            self._h = L.svih_setup_from_file(os.fsencode(path), C.byref(o))
        if not self._h:
            raise IOError("cannot read network %r" % (path,))
        self.link_thresh, self.lt_min_deg = link_thresh, lt_min_deg
        self.n = L.svih_n(self._h)
        self.k = L.svih_k(self._h)
        self.ones = L.svih_ones(self._h)
        self.singles = L.svih_singles(self._h)
        self.total_pairs = L.svih_total_pairs(self._h)
        self.ones_prob = L.svih_ones_prob(self._h)
        self.eta = (L.svih_eta0(self._h), L.svih_eta1(self._h))
        nv = L.svih_nvalidation(self._h)
        self.validation_sorted = _arr(L.svih_validation_sorted(self._h), (nv, 3), np.uint32)
        self.validation_accept = _arr(L.svih_validation_accept(self._h), (nv, 3), np.uint32)
        self.nlinks = L.svih_nlinks(self._h)
        self.links = _arr(L.svih_links(self._h), (self.nlinks, 2), np.uint32)
        self.seq2id = _arr(L.svih_seq2id(self._h), (self.n,), np.uint32)
        self.lam = _arr(L.svih_lambda(self._h), (self.k, 2), np.float64)

    @property
    def gamma(self):
        if not self.host_gamma:
            raise AttributeError("this Setup was made with host_gamma=False: gamma is drawn on the device (device_init)")
        return _arr(load().svih_gamma(self._h), (self.n, self.k), np.float64)

    def init_plan(self):
        """(streams, outputs per stream) as the drop-in binary cuts the init stream (host/linksampling.cc: init_gamma2_on_device)"""
        total = int(self.ones) * int(self.k)
        want = max(1, min(2048, total // (624 * 256)))
        per = ((total + want - 1) // want + 623) // 624 * 624
        return (total + per - 1) // per, per

    def device_init(self, eng, lam=None):
        """init_gamma2 on the device for `eng` (any handle: whole graph, node block, K-shard -- lam = its rows of lambda)"""
        if not hasattr(self, "_init_cache"):
            ns, per = self.init_plan()
            self._init_cache = (self.init_links(), self.init_streams(ns, per), per)
        edges, st, per = self._init_cache
        eng.init_gamma(edges, st, per, self.lam if lam is None else lam)

    @property
    def edges(self):
        return _arr(load().svih_edges(self._h), (self.ones, 2), np.uint32)

    def deg(self, p):
        return load().svih_deg(self._h, p)

    # ---- what svils_init_gamma takes (init_gamma2 on the device, csrc/svils_init.hip) ----
    def init_links(self):
        """every link (held-out ones included) in the order init_gamma2 draws for them: [E][2], p < q"""
        e = load().svih_init_links(self._h, None)
        out = np.empty((e, 2), dtype=np.uint32)
        load().svih_init_links(self._h, out.ctypes.data)
        return out

    def init_offset(self):
        """outputs the MT19937 stream had produced when init_gamma2 began (the held-out sampler's draws)"""
        return int(load().svih_init_offset(self._h))

    def init_streams(self, nstreams, per_stream):
        """[nstreams][624] MT19937 states, per_stream outputs apart, the first at init_offset() (jump-ahead, host/mtjump.hh)"""
        out = np.empty((nstreams, 624), dtype=np.uint32)
        if load().svih_init_streams(self._h, nstreams, per_stream, out.ctypes.data):
            raise RuntimeError("the jump-ahead machinery is unavailable")
        return out

    def engine(self, **kw):
        """An svils Engine loaded with this setup (graph, validation set, state)."""
        args = dict(ones=self.ones, ones_prob=self.ones_prob, eta=self.eta,
                    link_thresh=self.link_thresh, lt_min_deg=self.lt_min_deg)
        args.update(kw)
        eng = _svils.Engine(self.n, self.k, **args)
        eng.set_graph(self.links)
        eng.set_validation(self.validation_sorted)
        if self.host_gamma:
            eng.set_state(self.gamma, self.lam)
        else:
            self.device_init(eng)
        return eng

    def close(self):
        if getattr(self, "_h", None):
            load().svih_setup_free(self._h)
            self._h = None

    __del__ = close


class BatchEngine:
    """The `-batch` engine of the host library (svinet_amd/host/mmsbbatch.cc): the reference's
    all-pairs engine MMSBInfer::batch_infer (src/mmsbinfer.cc:833-930).  on_device=False: its host loops (plumbing only);
    on_device=True: the sweeps and pair likelihoods run through svils_batch_* on `device` (-batch-gpu) -- SvilsError
    without a HIP device, never the host loops instead.  sparse_graph=True (-sparse-graph): the sampled engines built on
    this class (SampledEngine, InfsetEngine, StratNodeEngine) on the device with the handle of svils_batch_create_sparse --
    no cap on n, no sweep and no lower bound; ValueError with on_device=False, logl=True or the all-pairs engine itself."""

    _SAMPLED = 0
    _STEP_SIZES = ("tau0", "kappa", "nodetau0", "nodekappa")   # the keyword arguments beyond the named ones

    def _open(self, L, path, o):
        """the engine's handle (a subclass with another constructor of the host library overrides this)"""
        return L.svih_batch_from_file(os.fsencode(path), C.byref(o))

    def __init__(self, path, n, k, seed=0, heldout_ratio=0.01, eta_type="uniform", on_device=False, device=0, nodelay=False,
                 logl=False, sparse_graph=False, **step_sizes):
        if sparse_graph and (type(self) is BatchEngine or not on_device or logl):
            raise ValueError("sparse_graph belongs to the sampled engines on the device: the all-pairs passes (a sweep, "
                             "the lower bound) need the dense form, and the host loops have no device graph")
        self.sparse_graph = bool(sparse_graph)
        L = load()
        vp, u32, u64, dbl, P = C.c_void_p, C.c_uint32, C.c_uint64, C.c_double, C.POINTER
        if not hasattr(L, "_batch_ready"):
            L.svih_batch_from_file.argtypes = [C.c_char_p, P(Options)]
            L.svih_batch_from_file.restype = vp
            for name, res in (("free", None), ("n", u32), ("iter", u32), ("gamma", P(dbl)), ("lambda", P(dbl)),
                              ("nheldout", u64), ("heldout", P(u32)), ("nvalidation", u64),
                              ("validation", P(u32)), ("nrows", u64), ("rows", P(dbl)), ("sweep", C.c_int),
                              ("report", C.c_int), ("eta0", dbl), ("eta1", dbl), ("ones_prob", dbl),
                              ("edges", P(u32)), ("ones", u32), ("nschedule", u64), ("total_pairs", dbl)):
                f = getattr(L, "svih_batch_" + name)
                f.argtypes = [vp]
                f.restype = res
            L.svih_batch_step.argtypes = [vp, u32]
            L.svih_batch_step.restype = C.c_int
            L.svih_batch_schedule.argtypes = [vp, u64, vp, vp]
            L.svih_batch_schedule.restype = u64
            L.svih_infset_from_file.argtypes = [C.c_char_p, C.c_char_p, P(Options)]
            L.svih_infset_from_file.restype = vp
            L.svih_batch_nstars.argtypes = [vp]
            L.svih_batch_nstars.restype = u64
            L.svih_batch_star.argtypes = [vp, u64, vp, vp, vp, vp]
            L.svih_batch_star.restype = u64
            for name in ("node_counts", "shuffled"):
                f = getattr(L, "svih_batch_" + name)
                f.argtypes = [vp]
                f.restype = P(u32)
            L.svih_batch_elbo.argtypes = [vp, vp]
            L.svih_batch_elbo.restype = C.c_int
            L.svih_batch_nlogl.argtypes = [vp]
            L.svih_batch_nlogl.restype = u64
            L.svih_batch_logl.argtypes = [vp]
            L.svih_batch_logl.restype = P(dbl)
            L._batch_ready = True
        o = Options()
        L.svih_options_default(C.byref(o), n, k)
        o.seed, o.heldout_ratio, o.eta_type = seed, heldout_ratio, ETA_TYPES[eta_type]
        o.batch_device, o.device = int(bool(on_device)), device
        o.sampled, o.nodelay = self._SAMPLED, int(bool(nodelay))
        o.logl = int(bool(logl))
        o.sparse_graph = int(bool(sparse_graph))
        for key, value in step_sizes.items():
            if key not in self._STEP_SIZES:
                raise TypeError("unexpected argument %r" % key)
            setattr(o, key, value)
        self._h = self._open(L, path, o)
        if not self._h:
            if on_device:   # (as FindK: an unreadable file and a failed svils_batch_* call both end here)
                err = _svils.load().svils_last_error().decode("utf-8", "replace")
                raise _svils.SvilsError(-2 if "no HIP device" in err else -1,
                                        "BatchEngine: cannot read %r or the device backend failed: %s" % (path, err))
            raise IOError("cannot read network %r" % (path,))
        self.n, self.k = L.svih_batch_n(self._h), k
        self.eta = (L.svih_batch_eta0(self._h), L.svih_batch_eta1(self._h))
        self.ones_prob = L.svih_batch_ones_prob(self._h)
        self.heldout = _arr(L.svih_batch_heldout(self._h), (L.svih_batch_nheldout(self._h), 2), np.uint32)
        self.validation = _arr(L.svih_batch_validation(self._h), (L.svih_batch_nvalidation(self._h), 2), np.uint32)
        self.edges = _arr(L.svih_batch_edges(self._h), (L.svih_batch_ones(self._h), 2), np.uint32)
        self.total_pairs = L.svih_batch_total_pairs(self._h)

    @property
    def gamma(self):
        return _arr(load().svih_batch_gamma(self._h), (self.n, self.k), np.float64)

    @property
    def lam(self):
        return _arr(load().svih_batch_lambda(self._h), (self.k, 2), np.float64)

    @property
    def rows(self):
        return _arr(load().svih_batch_rows(self._h), (load().svih_batch_nrows(self._h), 10), np.float64)

    @property
    def iter(self):
        return load().svih_batch_iter(self._h)

    def sweep(self):
        rc = load().svih_batch_sweep(self._h)
        if rc < 0:
            _svils._chk(rc)

    def report(self):
        rc = load().svih_batch_report(self._h)
        if rc < 0:
            _svils._chk(rc)
        return bool(rc)

    def elbo(self):
        """the variational lower bound of the current state (approx_log_likelihood, src/mmsbinfer.cc:1948-2056):
        (total, G, P, N).  on_device=True: svils_batch_elbo; else the host loops"""
        parts = np.empty(4)
        rc = load().svih_batch_elbo(self._h, parts.ctypes.data)
        if rc < 0:
            _svils._chk(rc)
        return tuple(parts)

    @property
    def logl_rows(self):
        """[rows][2] (iter, lower bound): with logl=True one row after the constructor and one per report"""
        return _arr(load().svih_batch_logl(self._h), (load().svih_batch_nlogl(self._h), 2), np.float64)

    def close(self):
        if getattr(self, "_h", None):
            load().svih_batch_free(self._h)
            self._h = None

    __del__ = close


def orig_stop_rule(seq, enabled=True):
    """The stop rules of -orig -logl (OrigStopRule, svinet_amd/host/mmsbinferorig.hh) driven over seq = [(iter, s), ...]:
    the verdict of every row -- 0 go on, 1 the drop rule (max.txt), 2 the gain rule (done.txt) -- stopping at the first stop"""
    L = load()
    L.svih_orig_stop_rule.argtypes = [C.c_void_p, C.c_uint32, C.c_double]
    L.svih_orig_stop_rule.restype = C.c_int32
    state = np.array([-np.finfo(np.float64).max, 0.0, 0.0, 1.0 if enabled else 0.0])
    out = []
    for it, s in seq:
        out.append(int(L.svih_orig_stop_rule(state.ctypes.data, int(it), float(s))))
        if out[-1]:
            break
    return out


class OrigEngine:
    """The `-orig` engine of the host library (svinet_amd/host/mmsbinferorig.cc): the reference's MMSBInferOrig::batch_infer
    (src/mmsbinferorig.cc:212-294), the blockmodel with a full K x K matrix of block rates.  on_device=True: the sweeps and
    pair likelihoods run through svils_orig_* on `device` -- SvilsError without a HIP device, never the host loops
    instead; on_device=False: the host loops (-host-loops).  clean_holdout=True (-clean-holdout): both orientations of every
    held-out and every validation pair are left out of training, not the held-out pairs in the drawn orientation alone.
    link_prob / predict_links / rank_links query the current state on the device (svils_orig_link_prob / _predict_links /
    _rank_links) and return what the _svils.Engine methods of the same names return."""

    def __init__(self, path, n, k, seed=0, heldout_ratio=0.01, itype=0, on_device=True, device=0, clean_holdout=False,
                 logl=False):
        L = load()
        vp, u32, u64, dbl, P = C.c_void_p, C.c_uint32, C.c_uint64, C.c_double, C.POINTER
        if not hasattr(L, "_orig_ready"):
            L.svih_orig_from_file.argtypes = [C.c_char_p, u32, u32, dbl, dbl, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
            L.svih_orig_device.argtypes = [vp]
            L.svih_orig_device.restype = vp
            L.svih_orig_from_file.restype = vp
            for name, res in (("free", None), ("n", u32), ("iter", u32), ("nheldout", u64), ("heldout", P(u32)),
                              ("nvalidation", u64), ("validation", P(u32)), ("nrows", u64), ("rows", P(dbl)),
                              ("rounds_total", u64), ("sweep", C.c_int), ("report", C.c_int), ("edges", P(u32)), ("ones", u32)):
                f = getattr(L, "svih_orig_" + name)
                f.argtypes = [vp]
                f.restype = res
            for name in ("gamma", "beta"):
                f = getattr(L, "svih_orig_" + name)
                f.argtypes = [vp, vp]
                f.restype = C.c_int
            L.svih_orig_set_state.argtypes = [vp, vp, vp]
            L.svih_orig_set_state.restype = C.c_int
            L.svih_orig_skip_also.argtypes = [vp, vp, u64]
            L.svih_orig_skip_also.restype = None
            L.svih_orig_from_file_logl.argtypes = L.svih_orig_from_file.argtypes + [C.c_int32]
            L.svih_orig_from_file_logl.restype = vp
            L.svih_orig_elbo.argtypes = [vp, vp, vp]
            L.svih_orig_elbo.restype = C.c_int
            L.svih_orig_nlogl_rows.argtypes = [vp]
            L.svih_orig_nlogl_rows.restype = u64
            L.svih_orig_logl_rows.argtypes = [vp]
            L.svih_orig_logl_rows.restype = P(dbl)
            L.svih_orig_stop_rule.argtypes = [vp, u32, dbl]
            L.svih_orig_stop_rule.restype = C.c_int32
            L._orig_ready = True
        self._h = L.svih_orig_from_file_logl(os.fsencode(path), n, k, seed, heldout_ratio, itype, int(bool(on_device)), device,
                                             int(bool(clean_holdout)), int(bool(logl)))
        if not self._h:
            if on_device:
                err = _svils.load().svils_last_error().decode("utf-8", "replace")
                raise _svils.SvilsError(-2 if "no HIP device" in err else -1,
                                        "OrigEngine: cannot read %r or the device backend failed: %s" % (path, err))
            raise IOError("cannot read network %r" % (path,))
        self.n, self.k = L.svih_orig_n(self._h), k
        self.heldout = _arr(L.svih_orig_heldout(self._h), (L.svih_orig_nheldout(self._h), 2), np.uint32)
        self.validation = _arr(L.svih_orig_validation(self._h), (L.svih_orig_nvalidation(self._h), 2), np.uint32)
        self.edges = _arr(L.svih_orig_edges(self._h), (L.svih_orig_ones(self._h), 2), np.uint32)

    def _device(self):
        h = load().svih_orig_device(self._h)
        if not h:
            raise _svils.SvilsError(-4, "OrigEngine: the link queries run on the device (on_device=True); the host loops have none")
        return _svils.Orig.borrowed(h, self.n, self.k)

    def link_prob(self, pairs):
        return self._device().link_prob(pairs)

    def predict_links(self, topk, nodes=None):
        return self._device().predict_links(topk, nodes)

    def rank_links(self, pairs):
        return self._device().rank_links(pairs)

    def _state(self, name, shape):
        out = np.empty(shape)
        rc = getattr(load(), "svih_orig_" + name)(self._h, out.ctypes.data)
        if rc < 0:
            _svils._chk(rc)
        return out

    @property
    def gamma(self):
        return self._state("gamma", (self.n, self.k))

    @property
    def beta(self):
        return self._state("beta", (self.k, self.k))

    @property
    def rows(self):
        """[rows][8]: which (0 held-out, 1 validation), iter, mean, count, mean of the non-links, count, mean of the links, count"""
        return _arr(load().svih_orig_rows(self._h), (load().svih_orig_nrows(self._h), 8), np.float64)

    @property
    def iter(self):
        return load().svih_orig_iter(self._h)

    @property
    def rounds_total(self):
        """host loops: the rounds over all pairs of the last sweep"""
        return load().svih_orig_rounds_total(self._h)

    def set_state(self, gamma, beta):
        gamma = np.ascontiguousarray(gamma, dtype=np.float64).reshape(self.n, self.k)
        beta = np.ascontiguousarray(beta, dtype=np.float64).reshape(self.k, self.k)
        rc = load().svih_orig_set_state(self._h, gamma.ctypes.data, beta.ctypes.data)
        if rc < 0:
            _svils._chk(rc)

    def skip_also(self, pairs):
        """host loops: leave these ordered pairs out as well (tests)"""
        pairs = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
        load().svih_orig_skip_also(self._h, pairs.ctypes.data, pairs.shape[0])

    def sweep(self):
        rc = load().svih_orig_sweep(self._h)
        if rc < 0:
            _svils._chk(rc)

    def report(self):
        rc = load().svih_orig_report(self._h)
        if rc < 0:
            _svils._chk(rc)

    def elbo(self):
        """the variational lower bound of the current state (approx_log_likelihood, src/mmsbinferorig.cc:624-726, over the
        pairs a sweep visits): (total, P, N).  on_device=True: svils_orig_elbo; else the host loops.  elbo_stats: (pairs,
        fixed-point rounds) of this pass"""
        out, st = np.empty(3), np.zeros(2, dtype=np.uint64)
        rc = load().svih_orig_elbo(self._h, out.ctypes.data, st.ctypes.data)
        if rc < 0:
            _svils._chk(rc)
        self.elbo_stats = (int(st[0]), int(st[1]))
        return tuple(out)

    @property
    def logl_rows(self):
        """[rows][2] (iter, lower bound): with logl=True one row after the constructor and one per report"""
        return _arr(load().svih_orig_logl_rows(self._h), (load().svih_orig_nlogl_rows(self._h), 2), np.float64)

    def close(self):
        if getattr(self, "_h", None):
            load().svih_orig_free(self._h)
            self._h = None

    __del__ = close


def sbm_rank_precision(pairs, score, y):
    """compute_precision's ranking (svinet_amd/host/sbm.cc: sbm_rank_precision) on its own: descending score, ties by
    ascending pair -> ((c10, c100, c1000) cumulative, curve [rows][2] of (rank, links so far))"""
    L = load()
    L.svih_sbm_rank_precision.argtypes = [C.c_void_p] * 3 + [C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64]
    L.svih_sbm_rank_precision.restype = C.c_uint64
    pairs = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
    score = np.ascontiguousarray(score, dtype=np.float64).reshape(-1)
    y = np.ascontiguousarray(y, dtype=np.uint8).reshape(-1)
    assert score.shape[0] == y.shape[0] == pairs.shape[0]
    cap = pairs.shape[0] // 1000 + 2
    out, curve = np.zeros(3, dtype=np.uint32), np.zeros((cap, 2), dtype=np.uint32)
    rows = L.svih_sbm_rank_precision(pairs.ctypes.data, score.ctypes.data, y.ctypes.data, pairs.shape[0], out.ctypes.data,
                                     curve.ctypes.data, cap)
    return tuple(int(v) for v in out), curve[:rows].copy()


class SbmEngine:
    """The `-single` engine of the host library (svinet_amd/host/sbm.cc): the reference's SBM::batch_infer (src/sbm.cc:457-543),
    the single-membership stochastic blockmodel.  on_device=True: every iteration and pair likelihood runs through svils_sbm_*
    on `device` -- SvilsError without a HIP device, never the host loops instead; on_device=False: the host loops
    (-host-loops).  heldout / validation / precision: the three samples [m][2], p < q, as drawn; skip: all of them, the pairs
    left out of training.  logl=True (-single-logl): every sweep() appends (iter, lower bound) to logl_rows after its M-step and
    sets stop_rule_verdict (0 go on, 1 the drop rule, 2 the gain rule; always 0 with stop=False, -no-stop); elbo() is the
    bound of the current state with or without it."""

    def __init__(self, path, n, k, seed=0, heldout_ratio=0.01, on_device=True, device=0, logl=False, stop=True):
        L = load()
        vp, u32, u64, dbl, P = C.c_void_p, C.c_uint32, C.c_uint64, C.c_double, C.POINTER
        if not hasattr(L, "_sbm_ready"):
            L.svih_sbm_from_file.argtypes = [C.c_char_p, u32, u32, dbl, dbl, C.c_int32, C.c_int32]
            L.svih_sbm_from_file.restype = vp
            for name, res in (("free", None), ("n", u32), ("iter", u32), ("passes", u32), ("msums", P(dbl)), ("nrows", u64),
                              ("rows", P(dbl)), ("sweep", C.c_int), ("edges", P(u32)), ("ones", u32)):
                f = getattr(L, "svih_sbm_" + name)
                f.argtypes = [vp]
                f.restype = res
            L.svih_sbm_state.argtypes = [vp, C.c_int32, vp]
            L.svih_sbm_state.restype = C.c_int
            L.svih_sbm_npairs.argtypes = [vp, C.c_int32]
            L.svih_sbm_npairs.restype = u64
            L.svih_sbm_pairs.argtypes = [vp, C.c_int32]
            L.svih_sbm_pairs.restype = P(u32)
            L.svih_sbm_set_state.argtypes = [vp, vp, vp, vp]
            L.svih_sbm_set_state.restype = C.c_int
            L.svih_sbm_from_file_logl.argtypes = L.svih_sbm_from_file.argtypes + [C.c_int32, C.c_int32]
            L.svih_sbm_from_file_logl.restype = vp
            L.svih_sbm_elbo.argtypes = [vp, vp]
            L.svih_sbm_elbo.restype = C.c_int
            L.svih_sbm_precision.argtypes = [vp, vp]
            L.svih_sbm_precision.restype = C.c_int
            L.svih_sbm_nlogl_rows.argtypes = [vp]
            L.svih_sbm_nlogl_rows.restype = u64
            L.svih_sbm_logl_rows.argtypes = [vp]
            L.svih_sbm_logl_rows.restype = P(dbl)
            L.svih_sbm_stop_rule_verdict.argtypes = [vp]
            L.svih_sbm_stop_rule_verdict.restype = C.c_int32
            L._sbm_ready = True
        self._h = L.svih_sbm_from_file_logl(os.fsencode(path), n, k, seed, heldout_ratio, int(bool(on_device)), device,
                                            int(bool(logl)), int(bool(stop)))
        if not self._h:
            if on_device:
                err = _svils.load().svils_last_error().decode("utf-8", "replace")
                raise _svils.SvilsError(-2 if "no HIP device" in err else -1,
                                        "SbmEngine: cannot read %r or the device backend failed: %s" % (path, err))
            raise IOError("cannot read network %r" % (path,))
        self.n, self.k = L.svih_sbm_n(self._h), k
        self.heldout, self.validation, self.precision = (
            _arr(L.svih_sbm_pairs(self._h, w), (L.svih_sbm_npairs(self._h, w), 2), np.uint32) for w in range(3))
        self.skip = np.concatenate([self.heldout, self.validation, self.precision])
        self.edges = _arr(L.svih_sbm_edges(self._h), (L.svih_sbm_ones(self._h), 2), np.uint32)

    def _state(self, which, shape):
        out = np.empty(shape)
        rc = load().svih_sbm_state(self._h, which, out.ctypes.data)
        if rc < 0:
            _svils._chk(rc)
        return out

    @property
    def phi(self):
        return self._state(0, (self.n, self.k))

    @property
    def gamma(self):
        return self._state(1, (self.k,))

    @property
    def lam(self):
        return self._state(2, (self.k + 1, 2))

    @property
    def eta(self):
        return self._state(3, (self.k + 1, 2))

    @property
    def rows(self):
        """[rows][8]: which (0 held-out, 1 validation), iter, mean, count, mean of the non-links, count, mean of the links, count;
        two rows after the constructor and two after every sweep()"""
        return _arr(load().svih_sbm_rows(self._h), (load().svih_sbm_nrows(self._h), 8), np.float64)

    @property
    def iter(self):
        return load().svih_sbm_iter(self._h)

    @property
    def passes(self):
        """passes of the last iteration's E-step"""
        return load().svih_sbm_passes(self._h)

    @property
    def msums(self):
        """msum of every pass of the last iteration's E-step"""
        return _arr(load().svih_sbm_msums(self._h), (self.passes,), np.float64)

    def set_state(self, phi, gamma, lam):
        phi = np.ascontiguousarray(phi, dtype=np.float64).reshape(self.n, self.k)
        gamma = np.ascontiguousarray(gamma, dtype=np.float64).reshape(self.k)
        lam = np.ascontiguousarray(lam, dtype=np.float64).reshape(self.k + 1, 2)
        rc = load().svih_sbm_set_state(self._h, phi.ctypes.data, gamma.ctypes.data, lam.ctypes.data)
        if rc < 0:
            _svils._chk(rc)

    def sweep(self):
        """one iteration: the E-step (at most 10 passes), the M-step, a held-out and a validation row"""
        rc = load().svih_sbm_sweep(self._h)
        if rc < 0:
            _svils._chk(rc)

    def elbo(self):
        """the variational lower bound of the current state (approx_log_likelihood, src/sbm.cc:1133-1239): (total, P, N, G).
        on_device=True: svils_sbmelbo; else the host loops over all pairs"""
        out = np.empty(4)
        rc = load().svih_sbm_elbo(self._h, out.ctypes.data)
        if rc < 0:
            _svils._chk(rc)
        return tuple(out)

    @property
    def logl_rows(self):
        """[rows][2] (iter, lower bound): with logl=True one row per sweep(), taken after its M-step"""
        return _arr(load().svih_sbm_logl_rows(self._h), (load().svih_sbm_nlogl_rows(self._h), 2), np.float64)

    @property
    def stop_rule_verdict(self):
        """the stop rules' answer to the last row: 0 go on, 1 the drop rule (max.txt), 2 the gain rule (done.txt)"""
        return int(load().svih_sbm_stop_rule_verdict(self._h))

    def feed_stop_rule(self, seq):
        """tests: the engine's own stop rule fed made-up rows seq = [(iter, s), ...] -> the verdict of every row, up to the first
        stop.  The rows do not enter logl_rows"""
        L = load()
        L.svih_sbm_feed_stop_rule.argtypes = [C.c_void_p, C.c_uint32, C.c_double]
        L.svih_sbm_feed_stop_rule.restype = C.c_int32
        out = []
        for it, s in seq:
            out.append(int(L.svih_sbm_feed_stop_rule(self._h, int(it), float(s))))
            if out[-1]:
                break
        return out

    def precision_counts(self):
        """compute_precision of the current state: the links among the first 10 / 100 / 1000 of the precision sample ranked by
        edge_likelihood2(p, q, 1) -> (c10, c100, c1000), cumulative"""
        out = np.zeros(3, dtype=np.uint32)
        rc = load().svih_sbm_precision(self._h, out.ctypes.data)
        if rc < 0:
            _svils._chk(rc)
        return tuple(int(v) for v in out)

    def close(self):
        if getattr(self, "_h", None):
            load().svih_sbm_free(self._h)
            self._h = None

    __del__ = close


class SampledEngine(BatchEngine):
    """The sampled-pair engines of the host library: the reference's MMSBInfer::infer (src/mmsbinfer.cc:459-740) for
    mode "rnode", "rpair" or "rpair-stratified".  on_device=False: its host loops (-host-loops); on_device=True: the steps
    and pair likelihoods run through svils_batch_step_* on `device`.  step(nsteps) draws nsteps iterations and runs them;
    schedule lists, per executed iteration, what was drawn: dict(node, family, pairs [m][2], scale, rho_gamma, rho_lambda)
    -- scale is the factor of gammat (n / 2, or scale / mbsize), rho_lambda < 0 an iteration that leaves lambda alone."""

    MODES = {"rnode": 1, "rpair": 2, "rpair-stratified": 3}

    def __init__(self, path, n, k, mode, on_device=False, nodelay=False, **kw):
        self._SAMPLED = self.MODES[mode]
        self.mode = mode
        super().__init__(path, n, k, on_device=on_device, nodelay=nodelay, **kw)

    def sweep(self):
        raise TypeError("a SampledEngine steps; BatchEngine sweeps")

    def step(self, nsteps=1):
        rc = load().svih_batch_step(self._h, nsteps)
        if rc < 0:
            _svils._chk(rc)

    @property
    def schedule(self):
        L, out = load(), []
        for i in range(L.svih_batch_nschedule(self._h)):
            head = np.zeros(5)
            m = L.svih_batch_schedule(self._h, i, head.ctypes.data, None)
            pairs = np.zeros((m, 2), dtype=np.uint32)
            L.svih_batch_schedule(self._h, i, None, pairs.ctypes.data)
            out.append(dict(node=int(head[0]), family=int(head[1]), pairs=pairs, scale=float(head[2]), rho_gamma=float(head[3]),
                            rho_lambda=float(head[4])))
        return out


def preprocess(path, n, out):
    """-preprocess: the informative sets of the graph of `path` (n declared nodes) written to `out` (neighbors.bin, the
    reference's format: per node uint32 id, 8-byte count, uint32 ids)"""
    L = load()
    L.svih_preprocess.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p]
    L.svih_preprocess.restype = C.c_int
    if L.svih_preprocess(os.fsencode(path), n, os.fsencode(out)) != 0:
        raise IOError("cannot read %r or write %r" % (path, out))


def read_neighbors(path, n):
    """the sets of a neighbors.bin -> list of n uint32 arrays"""
    raw = open(path, "rb").read()
    out, at = [], 0
    for i in range(n):
        node = int(np.frombuffer(raw, np.uint32, 1, at)[0])
        count = int(np.frombuffer(raw, np.uint64, 1, at + 4)[0])
        assert node == i
        out.append(np.frombuffer(raw, np.uint32, count, at + 12).copy())
        at += 12 + 4 * count
    assert at == len(raw)
    return out


class InfsetEngine(BatchEngine):
    """The -infset engine of the host library: the reference's FastAMM::infer (src/fastamm.cc:549-672), informative-set
    sampling, with the sets of `neighbors` (a neighbors.bin of preprocess()).  on_device=False: its host loops
    (-host-loops); on_device=True: the steps run through svils_batch_step_star on `device`, one call per step(nsteps).
    schedule lists, per executed iteration, what was drawn: dict(start, kind (0 links + informative set, 1
    non-informative), partner [m], y [m], rho_partner [m], rho_start, scale, rho_lambda); node_counts are the times every
    node's row was moved, shuffled the node order the non-informative steps walk.  inf_epsilon: the chance of kind 1."""

    _STEP_SIZES = BatchEngine._STEP_SIZES + ("inf_epsilon",)

    def __init__(self, path, n, k, neighbors, on_device=False, **kw):
        self._neighbors = neighbors
        super().__init__(path, n, k, on_device=on_device, **kw)

    def _open(self, L, path, o):
        return L.svih_infset_from_file(os.fsencode(path), os.fsencode(self._neighbors), C.byref(o))

    def sweep(self):
        raise TypeError("an InfsetEngine steps; BatchEngine sweeps")

    step = SampledEngine.step

    @property
    def schedule(self):
        L, out = load(), []
        for i in range(L.svih_batch_nstars(self._h)):
            head = np.zeros(5)
            m = L.svih_batch_star(self._h, i, head.ctypes.data, None, None, None)
            partner, y, rho = np.zeros(m, dtype=np.uint32), np.zeros(m, dtype=np.uint8), np.zeros(m)
            L.svih_batch_star(self._h, i, None, partner.ctypes.data, y.ctypes.data, rho.ctypes.data)
            out.append(dict(start=int(head[0]), kind=int(head[1]), partner=partner, y=y, rho_partner=rho, scale=float(head[2]),
                            rho_start=float(head[3]), rho_lambda=float(head[4])))
        return out

    @property
    def node_counts(self):
        return _arr(load().svih_batch_node_counts(self._h), (self.n,), np.uint32)

    @property
    def shuffled(self):
        return _arr(load().svih_batch_shuffled(self._h), (self.n,), np.uint32)


class StratNodeEngine(InfsetEngine):
    """The -snode engine of the host library: the reference's FastAMM2::infer (src/fastamm2.cc:535-702), the stratified
    random node sampler behind `-stratified -rnode`.  on_device=False: its host loops (-host-loops), which move all n rows
    at every iteration; on_device=True: the steps run through svils_batch_step_strat on `device`, one call per sweep() or
    step(nsteps).  sweep() runs one report interval (rfreq iterations, 100 as the CLI's default).  schedule() lists, per
    executed iteration, what was drawn: dict(start, kind (0 links, 1 a block of non-links), partner [m], y [m], rho_gamma,
    scale, rho_lambda); shuffled() is the node order the non-link steps walk.  inf_epsilon: the chance of kind 1 (0.5)."""

    def __init__(self, path, n, k, on_device=False, rfreq=100, inf_epsilon=0.5, **kw):
        self.rfreq = rfreq
        BatchEngine.__init__(self, path, n, k, on_device=on_device, inf_epsilon=inf_epsilon, **kw)

    def _open(self, L, path, o):
        L.svih_snode_from_file.argtypes = [C.c_char_p, C.POINTER(Options)]
        L.svih_snode_from_file.restype = C.c_void_p
        return L.svih_snode_from_file(os.fsencode(path), C.byref(o))

    def sweep(self):
        """one report interval: rfreq iterations drawn, then run (on the device: one svils_batch_step_strat call)"""
        self.step(self.rfreq)

    def schedule(self):
        out = []
        for d in InfsetEngine.schedule.fget(self):
            rho = d.pop("rho_start")
            assert np.all(d.pop("rho_partner") == rho)
            d["rho_gamma"] = rho
            out.append(d)
        return out

    def shuffled(self):
        return InfsetEngine.shuffled.fget(self)

    node_counts = None   # FastAMM2 counts every node at every iteration: the count is iter


class FindK:
    """-findk on the device (svils_findk_*), driven by the product's host side (host/findk.cc: init_gamma, the held-out
    sample, the padding draws) with nothing written to disk.  step() runs one pass of the reference's batch_infer loop
    (src/fastinit.cc:240-289): 0 = an iteration with its groups, 1 = the held-out stop rule fired (no groups), 2 = the loop
    was already over.  -seed does not enter: FastInit draws from the default stream."""

    STEP_ITERATION, STEP_STOPPED, STEP_DONE = 0, 1, 2

    def __init__(self, path=None, n=0, k=0, pairs=None, heldout_ratio=0.01, link_thresh=0.5, accuracy=False, device=0):
        L = load()
        o = Options()
        L.svih_options_default(C.byref(o), n, k)
        o.heldout_ratio = heldout_ratio
        o.link_thresh = link_thresh
        o.accuracy = int(accuracy)
        if pairs is not None:
            pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
            self._h = L.svih_findk_from_pairs(pairs.ctypes.data, pairs.shape[0], C.byref(o), device)
        else:
            self._h = L.svih_findk_from_file(os.fsencode(path), C.byref(o), device)
        if not self._h:
            raise RuntimeError("FindK: cannot read %r or no device: %s" % (path, _svils.load().svils_last_error().decode()))
        self.n = L.svih_findk_n(self._h)
        self.seq2id = _arr(L.svih_findk_seq2id(self._h), (self.n,), np.uint32)
        self.heldout = _arr(L.svih_findk_heldout(self._h), (L.svih_findk_nheldout(self._h), 3), np.uint32)

    def step(self):
        rc = load().svih_findk_step(self._h)
        if rc < 0:
            _svils._chk(rc)
        return rc

    def run(self):
        """every pass until the loop ends; returns the heldout.txt rows (11 columns each)"""
        rows = []
        while True:
            r = self.step()
            if r == self.STEP_DONE:
                return np.array(rows).reshape(-1, 11)
            rows.append(self.row)
            if r == self.STEP_STOPPED:
                return np.array(rows).reshape(-1, 11)

    def state(self):
        """(labels [n][5] uint32, values [n][5] float64, masks [n] uint32) after the last step"""
        lab = np.zeros((self.n, 5), np.uint32)
        val = np.zeros((self.n, 5), np.float64)
        mk = np.zeros(self.n, np.uint32)
        load().svih_findk_state(self._h, lab.ctypes.data, val.ctypes.data, mk.ctypes.data)
        return lab, val, mk

    @property
    def row(self):
        r = np.zeros(11, np.float64)
        load().svih_findk_row(self._h, r.ctypes.data)
        return r

    @property
    def iter(self):
        return load().svih_findk_iter(self._h)

    @property
    def unlikely(self):
        return load().svih_findk_unlikely(self._h)

    @property
    def training_ll(self):
        return load().svih_findk_training_ll(self._h)

    def timing(self):
        """device ms of the last step's count, apply, likelihoods, groups; the host padding seconds; the padded nodes"""
        ms = np.zeros(4, np.float64)
        load().svih_findk_timing(self._h, ms.ctypes.data)
        return {"count_ms": ms[0], "apply_ms": ms[1], "likelihood_ms": ms[2], "groups_ms": ms[3],
                "pad_host_ms": 1e3 * load().svih_findk_pad_seconds(self._h), "npad": load().svih_findk_npad(self._h)}

    def close(self):
        if getattr(self, "_h", None):
            load().svih_findk_free(self._h)
            self._h = None

    __del__ = close


def LinkCommunities(links, gamma, lam, device=0, with_pi=False):
    """-gml / -lcstats on the device (svils_lc_*) with nothing written to disk: the reference's MMSBGen::get_lc_stats and
    gml (src/mmsbgen.cc:181-193, 911-961) for the model gamma [n][k], lam [k][2].  `links` is a [E][2] array of sequence
    ids (p < q, every link of the network) or the path of an edge list, read with the product's reader (n = the rows of
    gamma).  Returns a dict of numpy arrays: per node group, bridgeness, memberships, influence; deg_c [n][k]; per
    community comm_nodes, comm_degsum, comm_max, comm_argmax; per link (in the given order) colour, join, gml, rechecked;
    gml_edges [m][3] (p, q, colour) in (p, q) order; the counts unlikely / rechecked; timing_ms (node, link, count passes);
    with_pi: pi [n][k]."""
    gamma = np.ascontiguousarray(gamma, dtype=np.float64)
    lam = np.ascontiguousarray(lam, dtype=np.float64).reshape(-1, 2)
    n, k = gamma.shape
    out = {}
    if isinstance(links, (str, bytes, os.PathLike)):
        s = Setup(links, n, k, host_gamma=False)
        try:
            if s.n != n:
                raise ValueError("the network has %d nodes with links; gamma has %d rows" % (s.n, n))
            links, out["seq2id"] = s.edges, s.seq2id
        finally:
            s.close()
    links = np.ascontiguousarray(links, dtype=np.uint32).reshape(-1, 2)
    if lam.shape[0] != k:
        raise ValueError("lam has %d rows; gamma has %d columns" % (lam.shape[0], k))
    L = _svils.load()
    E = links.shape[0]
    ok = _svils._chk
    h = C.c_void_p()
    ok(L.svils_lc_create(device, n, k, C.byref(h)))
    try:
        ok(L.svils_lc_set_graph(h, links.ctypes.data, E))
        ok(L.svils_lc_set_model(h, gamma.ctypes.data, lam.ctypes.data))
        ok(L.svils_lc_run(h))
        for name in ("group", "memberships", "influence"):
            out[name] = np.zeros(n, np.uint32)
        out["bridgeness"] = np.zeros(n, np.float64)
        ok(L.svils_lc_get_nodes(h, out["group"].ctypes.data, out["bridgeness"].ctypes.data, out["memberships"].ctypes.data,
                                out["influence"].ctypes.data))
        out["deg_c"] = np.zeros((n, k), np.uint32)
        ok(L.svils_lc_get_degrees(h, out["deg_c"].ctypes.data))
        if with_pi:
            out["pi"] = np.zeros((n, k), np.float64)
            ok(L.svils_lc_get_pi(h, out["pi"].ctypes.data))
        out["comm_nodes"], out["comm_degsum"] = np.zeros(k, np.uint32), np.zeros(k, np.uint64)
        out["comm_max"], out["comm_argmax"] = np.zeros(k, np.uint32), np.zeros(k, np.uint32)
        ok(L.svils_lc_get_communities(h, out["comm_nodes"].ctypes.data, out["comm_degsum"].ctypes.data, out["comm_max"].ctypes.data,
                                      out["comm_argmax"].ctypes.data))
        colour, flags, counts = np.zeros(E, np.uint32), np.zeros(E, np.uint8), np.zeros(3, np.uint64)
        ok(L.svils_lc_get_links(h, colour.ctypes.data, flags.ctypes.data, counts.ctypes.data))
        out["colour"] = colour
        out["join"], out["gml"], out["rechecked"] = (flags & 1) != 0, (flags & 2) != 0, (flags & 4) != 0
        out["unlikely"], out["n_rechecked"] = int(counts[0]), int(counts[2])
        out["gml_edges"] = np.zeros((int(counts[1]), 3), np.uint32)
        m = C.c_uint64()
        ok(L.svils_lc_get_gml(h, C.byref(m), out["gml_edges"].ctypes.data))
        ms = np.zeros(3, np.float64)
        ok(L.svils_lc_get_timing(h, ms.ctypes.data))
        out["timing_ms"] = {"node": ms[0], "link": ms[1], "count": ms[2]}
        out["links"] = links
    finally:
        L.svils_lc_destroy(h)
    return out


class PPC:
    """One svils_ppc handle: networks drawn from a model (pi [n][k], beta [k]) and the statistics of a link list, the device
    side of the reference's MMSBGen::gen and MMSBGen::ppc (src/mmsbgen.cc:43-71, 662-697).  The draw is the library's own
    definition (include/svils.h), not GSL's stream.  max_links: the room of the link list (default:
    every pair).

        ppc = PPC(n, k); links = ppc.draw(pi, beta, seed, r); rep = ppc.stats()
        ppc.observe(observed_links); obs = ppc.stats()

    The same handle serves the K x K blockmodel of -orig: set_params_orig(pi, B) or draw(pi, B=B, ...)
    makes that kind current, set_params(pi, beta) the assortative one; the last call decides."""

    def __init__(self, n, k, device=0, max_links=None):
        self._h = C.c_void_p()
        self.n, self.k = int(n), int(k)
        if max_links is None:
            max_links = self.n * (self.n - 1) // 2
        self.blocks = False          # the K x K kind is current
        _svils._chk(_svils.load().svils_ppc_create(device, self.n, self.k, int(max_links), C.byref(self._h)))

    def set_params(self, pi, beta):
        pi = np.ascontiguousarray(pi, dtype=np.float64)
        beta = np.ascontiguousarray(beta, dtype=np.float64).reshape(-1)
        if pi.shape != (self.n, self.k) or beta.shape != (self.k,):
            raise ValueError("pi must be [%d][%d] and beta [%d]" % (self.n, self.k, self.k))
        _svils._chk(_svils.load().svils_ppc_set_params(self._h, pi.ctypes.data, beta.ctypes.data))
        self.blocks = False

    def set_params_orig(self, pi, B):
        """the K x K kind: pi [n][k] and the block rates B [k][k] in [0, 1] (row g: the smaller node id's block)"""
        pi = np.ascontiguousarray(pi, dtype=np.float64)
        B = np.ascontiguousarray(B, dtype=np.float64)
        if pi.shape != (self.n, self.k) or B.shape != (self.k, self.k):
            raise ValueError("pi must be [%d][%d] and B [%d][%d]" % (self.n, self.k, self.k, self.k))
        _svils._chk(_svils.load().svils_ppc_set_params_orig(self._h, pi.ctypes.data, B.ctypes.data))
        self.blocks = True

    def set_tile_batch(self, tiles_per_launch):
        """tiles per launch of the draw (0: one launch); no result depends on it"""
        _svils._chk(_svils.load().svils_ppc_set_tile_batch(self._h, int(tiles_per_launch)))

    def draw(self, pi=None, beta=None, seed=0, r=0, B=None):
        """replicate r of seed under (pi, beta), or under (pi, B) of the K x K kind (None: the parameters set last), becomes
        the current list -> links [E][2]"""
        if pi is not None and B is not None:
            self.set_params_orig(pi, B)
        elif pi is not None:
            self.set_params(pi, beta)
        _svils._chk(_svils.load().svils_ppc_draw(self._h, int(seed), int(r)))
        return self.links()

    def draw_counts(self):
        """(links of the last draw -- also of one that did not fit the list --, pairs it rechecked)"""
        c = np.zeros(2, np.uint64)
        _svils._chk(_svils.load().svils_ppc_get_draw_counts(self._h, c.ctypes.data))
        return int(c[0]), int(c[1])

    def observe(self, links):
        """the observed network (links [E][2], p < q, no repeats) becomes the current list"""
        links = np.ascontiguousarray(links, dtype=np.uint32).reshape(-1, 2)
        _svils._chk(_svils.load().svils_ppc_set_links(self._h, links.ctypes.data, links.shape[0]))

    def links(self):
        m = C.c_uint64()
        L = _svils.load()
        _svils._chk(L.svils_ppc_get_links(self._h, C.byref(m), None, None, None))
        out = np.zeros((m.value, 2), np.uint32)
        _svils._chk(L.svils_ppc_get_links(self._h, C.byref(m), out.ctypes.data, None, None))
        return out

    def stats(self):
        """the statistics of the current list under the current parameters, as a dict: links [E][2] in (p, q) order with
        colour and join per link; deg, tri [n]; ones, max_deg, argmax_deg, triangles, wedges, transitivity, clustering;
        size, logpe [k]; rechecked (pairs of the last draw); timing_ms (draw, csr, stats).  Under the K x K kind colour is
        g k + h and block_size, block_logpe [k][k] and offdiag_share (joined links in blocks g != h / joined links, NaN
        without one) stand in place of size and logpe"""
        L, ok = _svils.load(), _svils._chk
        ok(L.svils_ppc_stats(self._h))
        out = {"links": self.links()}
        E = out["links"].shape[0]
        colour, joined = np.zeros(E, np.uint32), np.zeros(E, np.uint8)
        m = C.c_uint64()
        ok(L.svils_ppc_get_links(self._h, C.byref(m), None, colour.ctypes.data, joined.ctypes.data))
        out["colour"], out["join"] = colour, joined != 0
        out["deg"], out["tri"] = np.zeros(self.n, np.uint32), np.zeros(self.n, np.uint32)
        ok(L.svils_ppc_get_nodes(self._h, out["deg"].ctypes.data, out["tri"].ctypes.data))
        counts, values = np.zeros(5, np.uint64), np.zeros(2, np.float64)
        ok(L.svils_ppc_get_summary(self._h, counts.ctypes.data, values.ctypes.data))
        for name, v in zip(("ones", "max_deg", "argmax_deg", "triangles", "wedges"), counts):
            out[name] = int(v)
        out["transitivity"], out["clustering"] = float(values[0]), float(values[1])
        if self.blocks:
            bs, bl = np.zeros((self.k, self.k), np.uint64), np.zeros((self.k, self.k), np.float64)
            ok(L.svils_ppc_get_blocks(self._h, bs.ctypes.data, bl.ctypes.data))
            joined = int(bs.sum())
            out["block_size"], out["block_logpe"] = bs, bl
            out["offdiag_share"] = float(joined - int(np.trace(bs))) / float(joined) if joined else float("nan")
        else:
            out["size"], out["logpe"] = np.zeros(self.k, np.uint64), np.zeros(self.k, np.float64)
            ok(L.svils_ppc_get_communities(self._h, out["size"].ctypes.data, out["logpe"].ctypes.data))
        out["rechecked"] = self.draw_counts()[1]
        ms = np.zeros(3, np.float64)
        ok(L.svils_ppc_get_timing(self._h, ms.ctypes.data))
        out["timing_ms"] = {"draw": ms[0], "csr": ms[1], "stats": ms[2]}
        return out

    def set_hop_batch(self, words=0, levels_per_chunk=0):
        """64-bit words per node of a BFS pass (1 .. 8; a pass runs 64 x words sources) and the levels queued between two
        reads of the level counter; 0: the default.  No result depends on it"""
        _svils._chk(_svils.load().svils_ppc_set_hop_batch(self._h, int(words), int(levels_per_chunk)))

    def hops(self):
        """the exact hop plot and the components of the current list, as a dict: D [levels] (ordered
        pairs at distance h, D[0] = n), ecc, comp [n]; effdiam, meandist; reachable, diameter, components, largest, isolated"""
        L, ok = _svils.load(), _svils._chk
        ok(L.svils_ppc_hops(self._h))
        counts, values = np.zeros(6, np.uint64), np.zeros(2, np.float64)
        ok(L.svils_ppc_get_hop_summary(self._h, counts.ctypes.data, values.ctypes.data))
        out = {"D": np.zeros(int(counts[5]), np.uint64), "ecc": np.zeros(self.n, np.uint32), "comp": np.zeros(self.n, np.uint32)}
        levels = C.c_uint32()
        ok(L.svils_ppc_get_hops(self._h, C.byref(levels), out["D"].ctypes.data, out["D"].shape[0]))
        ok(L.svils_ppc_get_hop_nodes(self._h, out["ecc"].ctypes.data, out["comp"].ctypes.data))
        out["effdiam"], out["meandist"] = float(values[0]), float(values[1])
        for name, v in zip(("reachable", "diameter", "components", "largest", "isolated"), counts):
            out[name] = int(v)
        return out

    def hop_timing(self):
        """(device ms of the last hops(), kernel launches it queued); (-1, -1) before the first"""
        ms = np.zeros(2, np.float64)
        _svils._chk(_svils.load().svils_ppc_get_hop_timing(self._h, ms.ctypes.data))
        return float(ms[0]), int(ms[1])

    def close(self):
        if getattr(self, "_h", None):
            _svils.load().svils_ppc_destroy(self._h)
            self._h = None

    __del__ = close


def ppc_philox(counters, key):
    """the host side's Philox4x32-10 (host/ppc.cc) of counters [m][4] under key (k0, k1) -> uint32 [m][4]"""
    c = np.ascontiguousarray(counters, dtype=np.uint32).reshape(-1, 4)
    k = np.ascontiguousarray(key, dtype=np.uint32).reshape(2)
    out = np.zeros_like(c)
    load().svih_ppc_philox(c.ctypes.data, c.shape[0], k.ctypes.data, out.ctypes.data)
    return out


def ppc_params(gamma, lam, seed, r):
    """the parameters of replicate r of seed as -ppc draws them on the host: pi_i ~ Dirichlet(gamma_i) [n][k],
    beta_k ~ Beta(lam_k0, lam_k1) [k] (MMSBGen::draw_all, src/mmsbgen.cc:730-742, over this project's Philox streams)"""
    gamma = np.ascontiguousarray(gamma, dtype=np.float64)
    lam = np.ascontiguousarray(lam, dtype=np.float64).reshape(-1, 2)
    n, k = gamma.shape
    assert lam.shape[0] == k
    pi, beta = np.zeros((n, k)), np.zeros(k)
    load().svih_ppc_dirichlet(gamma.ctypes.data, n, k, int(seed), int(r), pi.ctypes.data)
    load().svih_ppc_beta(lam.ctypes.data, k, int(seed), int(r), beta.ctypes.data)
    return pi, beta
