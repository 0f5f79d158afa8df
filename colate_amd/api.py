"""Thin Python face of the C ABI (include/colate_amd.h).  numpy arrays for the host-pointer
entry points, torch CUDA(=HIP) tensors for the *_device ones."""
import ctypes

import numpy as np

from ._lib import ColateError, c_char_p, c_int, check, lib  # noqa: F401

FLAG_NAN, FLAG_NEG, FLAG_MAXITER, FLAG_UNRESOLVED = 1, 2, 4, 8
STATUS_MASK = 0x07  # the error-like bits of out_flags (NaN / negative / iteration cap)
DEFAULT_MAX_ITER = 100000
DEFAULT_MIN_ITER = 1000
DEFAULT_REL_TOL = 1e-7
DEFAULT_RATE_FLOOR = 5e-9
DEFAULT_INIT_RATE = 1.0 / 20000.0
MAX_EPOCHS = 1024


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a):
    return a.ctypes.data


def version():
    return lib.colate_version().decode()


def device_count():
    return lib.colate_device_count()


def unresolved_epochs(flags):
    """COLATE_UNRESOLVED_EPOCHS: how many trailing epochs of each replicate are below the resolution of the
    reference's arithmetic (include/colate_amd.h, COLATE_FLAG_UNRESOLVED)."""
    return (np.asarray(flags).astype(np.int64) & 0xFFFFFFFF) >> 8


def status_flags(flags):
    """The error-like bits of out_flags (NaN / negative / iteration cap); 0 = the replicate ran clean."""
    return np.asarray(flags) & STATUS_MASK


EM_VARIANTS = ("latency-ilp", "latency", "throughput")


def em_kernel_variant(B, E):
    """Which build of the EM kernel a batch of this shape runs on the current device."""
    return EM_VARIANTS[check(lib.colate_em_kernel_variant(int(B), int(E)))]


def em_force_variant(name=None):
    """Force the build of the EM kernel for E <= 128 ("latency-ilp", "latency", "throughput"); None = automatic."""
    check(lib.colate_em_force_variant(-1 if name is None else EM_VARIANTS.index(name)))


def em_kernel_build(B, E):
    """The instantiation of the EM kernel a fit of B replicates x E epochs runs on the current device, under the current
    forcing: `unit-kind/NCHxEROWS`, e.g. "ilp-capped/1x4" (include/colate_amd.h, colate_em_kernel_build)."""
    name = ctypes.create_string_buffer(64)
    check(lib.colate_em_kernel_build(int(B), int(E), name, 64))
    return name.value.decode()


def em_kernel_build_for(B, E, cus, forced=None, mode=0):
    """The same from given numbers, without a device: `cus` compute units (0 = unknown), `forced` one of EM_VARIANTS or
    None, mode 0 = EM fit, 1 = one E-step."""
    name = ctypes.create_string_buffer(64)
    check(lib.colate_em_kernel_build_for(int(mode), int(B), int(E), int(cus), -1 if forced is None else EM_VARIANTS.index(forced),
                                         name, 64))
    return name.value.decode()


def em_kernel_builds(mode=0):
    """Every name the dispatch can return for `mode`, in the table's order."""
    buf = ctypes.create_string_buffer(2048)
    check(lib.colate_em_kernel_builds(int(mode), buf, 2048))
    return buf.value.decode().split("\n")


def age_grid():
    """coal.cpp:3126-3137."""
    g = np.zeros(256)
    n = check(lib.colate_age_grid(_p(g), 256))
    return g[:n].copy()


def epochs_from_bins(bins, age=0.0, years_per_gen=28.0):
    """coal.cpp:3551-3632.  Returns (epochs, ep_null)."""
    ep = np.zeros(MAX_EPOCHS)
    en = c_int(0)
    n = check(lib.colate_epochs_from_bins(bins.encode(), age, years_per_gen, _p(ep), MAX_EPOCHS, ctypes.byref(en)))
    return ep[:n].copy(), en.value


def epochs_from_coal(path, age=0.0):
    """coal.cpp:3508-3549, 3638-3646.  Returns (epochs, init_rates)."""
    ep = np.zeros(MAX_EPOCHS)
    r = np.zeros(MAX_EPOCHS)
    n = check(lib.colate_epochs_from_coal(str(path).encode(), age, _p(ep), _p(r), MAX_EPOCHS))
    return ep[:n].copy(), r[:n].copy()


class Rng:
    """std::mt19937 handle (coal.cpp:3157-3162)."""

    def __init__(self, seed):
        self.h = lib.colate_rng_create(seed)

    def __del__(self):
        if getattr(self, "h", None):
            lib.colate_rng_destroy(self.h)
            self.h = None


def bootstrap_counts(rng, num_bootstrap, age_grid_, age, sh_block, ns_block, sh_emp_block, ns_emp_block):
    """coal.cpp:3344-3451.  Block tables are [nb][A].  Returns (cnt_shared[B][A], cnt_notshared[B][A])."""
    g = _f64(age_grid_)
    t = [_f64(x) for x in (sh_block, ns_block, sh_emp_block, ns_emp_block)]
    nb, A = t[0].shape
    csh = np.zeros((num_bootstrap, A))
    cns = np.zeros((num_bootstrap, A))
    check(lib.colate_bootstrap_counts(rng.h, num_bootstrap, nb, A, _p(g), age, _p(t[0]), _p(t[1]), _p(t[2]),
                                      _p(t[3]), _p(csh), _p(cns)))
    return csh, cns


def bootstrap_weights(rng, num_bootstrap, nb):
    """coal.cpp:3350-3357: multinomial block weights [num_bootstrap][nb] from the shared mt19937."""
    w = np.zeros((num_bootstrap, nb))
    check(lib.colate_bootstrap_weights(rng.h, num_bootstrap, nb, _p(w)))
    return w


def bootstrap_counts_device(age_grid_, age, weights, sh_block, ns_block, sh_emp_block, ns_emp_block, cnt_shared,
                            cnt_notshared, stream=None):
    """colate_bootstrap_counts_device on torch tensors in HBM (float64, contiguous); asynchronous."""
    B, nb = weights.shape
    A = age_grid_.numel()
    for t in (age_grid_, weights, sh_block, ns_block, sh_emp_block, ns_emp_block, cnt_shared, cnt_notshared):
        assert t.is_cuda and t.is_contiguous()
    import torch

    status = torch.zeros(1, dtype=torch.int32, device=weights.device)
    check(lib.colate_bootstrap_counts_device(B, nb, A, age_grid_.data_ptr(), float(age), weights.data_ptr(),
                                             sh_block.data_ptr(), ns_block.data_ptr(), sh_emp_block.data_ptr(),
                                             ns_emp_block.data_ptr(), cnt_shared.data_ptr(), cnt_notshared.data_ptr(),
                                             status.data_ptr(), _stream_ptr(stream)))
    return status


def bootstrap_counts_from_weights(age_grid_, age, weights, sh_block, ns_block, sh_emp_block, ns_emp_block):
    """coal.cpp:3358-3451 on the host from given weights[B][nb] (the host twin of the GPU bootstrap)."""
    g, w = _f64(age_grid_), _f64(np.atleast_2d(weights))
    t = [_f64(x) for x in (sh_block, ns_block, sh_emp_block, ns_emp_block)]
    nb, A = t[0].shape
    B = w.shape[0]
    assert w.shape == (B, nb)
    csh = np.zeros((B, A))
    cns = np.zeros((B, A))
    check(lib.colate_bootstrap_counts_from_weights(B, nb, A, _p(g), float(age), _p(w), _p(t[0]), _p(t[1]), _p(t[2]), _p(t[3]),
                                                   _p(csh), _p(cns)))
    return csh, cns


def _lead(devices):
    """The (num_devices, devices) arguments in front of a *_sharded call; none for the one-device call."""
    if devices is None:
        return ()
    dev = np.ascontiguousarray(devices, dtype=np.int32)
    return dev.size, _p(dev), dev  # (the array itself rides along so that it outlives the call)


def _bootstrap_em_batch(devices, age_grid_, age, weights, sh_block, ns_block, sh_emp_block, ns_emp_block, epochs, init_rates,
                        max_iter, min_iter, rel_tol, rate_floor, want_counts):
    g, w, ep = _f64(age_grid_), _f64(np.atleast_2d(weights)), _f64(epochs)
    t = [_f64(x) for x in (sh_block, ns_block, sh_emp_block, ns_emp_block)]
    nb, A = t[0].shape
    B, E = w.shape[0], ep.size
    init = _f64(np.full(E, DEFAULT_INIT_RATE) if init_rates is None else init_rates)
    rates, iters, ll, flags = np.zeros((B, E)), np.zeros(B, dtype=np.int32), np.zeros(B), np.zeros(B, dtype=np.int32)
    csh, cns = (np.zeros((B, A)), np.zeros((B, A))) if want_counts else (None, None)
    lead = _lead(devices)
    f = lib.colate_bootstrap_em_batch if devices is None else lib.colate_bootstrap_em_batch_sharded
    check(f(*lead[:2], B, nb, E, A, _p(g), float(age), _p(w), _p(t[0]), _p(t[1]), _p(t[2]), _p(t[3]), _p(ep), _p(init), max_iter,
            min_iter, rel_tol, rate_floor, _p(rates), _p(iters), _p(ll), _p(flags), _p(csh) if want_counts else None,
            _p(cns) if want_counts else None))
    return (rates, iters, ll, flags, csh, cns) if want_counts else (rates, iters, ll, flags)


def bootstrap_em_batch(age_grid_, age, weights, sh_block, ns_block, sh_emp_block, ns_emp_block, epochs, init_rates=None,
                       max_iter=DEFAULT_MAX_ITER, min_iter=DEFAULT_MIN_ITER, rel_tol=DEFAULT_REL_TOL,
                       rate_floor=DEFAULT_RATE_FLOOR, want_counts=False):
    """colate_bootstrap_em_batch: block tables [nb][A] + weights [B][nb] -> (rates, iters, loglik, flags[, csh, cns])."""
    return _bootstrap_em_batch(None, age_grid_, age, weights, sh_block, ns_block, sh_emp_block, ns_emp_block, epochs, init_rates,
                               max_iter, min_iter, rel_tol, rate_floor, want_counts)


def bootstrap_em_batch_sharded(devices, age_grid_, age, weights, sh_block, ns_block, sh_emp_block, ns_emp_block, epochs,
                               init_rates=None, max_iter=DEFAULT_MAX_ITER, min_iter=DEFAULT_MIN_ITER, rel_tol=DEFAULT_REL_TOL,
                               rate_floor=DEFAULT_RATE_FLOOR, want_counts=False):
    """colate_bootstrap_em_batch_sharded: bootstrap_em_batch with the replicates sharded over the GPUs listed in `devices`
    (ordinals may repeat)."""
    return _bootstrap_em_batch(devices, age_grid_, age, weights, sh_block, ns_block, sh_emp_block, ns_emp_block, epochs,
                               init_rates, max_iter, min_iter, rel_tol, rate_floor, want_counts)


def _bootstrap_em_batch_groups(devices, age_grid_, ages, weights, tables, epochs, init_rates, max_iter, min_iter, rel_tol,
                               rate_floor, want_counts):
    g = _f64(age_grid_)
    G = len(weights)
    ws = [_f64(np.atleast_2d(w)) for w in weights]
    B = ws[0].shape[0]
    nb = np.ascontiguousarray([w.shape[1] for w in ws], dtype=np.int32)
    assert all(w.shape[0] == B for w in ws)
    ep = _f64(np.atleast_2d(epochs))
    E, A = ep.shape[1], g.size
    assert ep.shape == (G, E)
    init = _f64(np.full((G, E), DEFAULT_INIT_RATE) if init_rates is None else np.atleast_2d(init_rates))
    w_all = _f64(np.concatenate([w.ravel() for w in ws]))
    t_all = [_f64(np.concatenate([_f64(tables[k][j]).reshape(-1, A) for k in range(G)])) for j in range(4)]
    assert all(t.shape == (int(nb.sum()), A) for t in t_all)
    a = _f64(ages)
    R = G * B
    rates, iters, ll, flags = np.zeros((R, E)), np.zeros(R, dtype=np.int32), np.zeros(R), np.zeros(R, dtype=np.int32)
    csh, cns = (np.zeros((R, A)), np.zeros((R, A))) if want_counts else (None, None)
    lead = _lead(devices)
    f = lib.colate_bootstrap_em_batch_groups if devices is None else lib.colate_bootstrap_em_batch_groups_sharded
    check(f(*lead[:2], G, B, E, A, _p(g), _p(nb), _p(a), _p(w_all), _p(t_all[0]), _p(t_all[1]), _p(t_all[2]), _p(t_all[3]), _p(ep),
            _p(init), max_iter, min_iter, rel_tol, rate_floor, _p(rates), _p(iters), _p(ll), _p(flags),
            _p(csh) if want_counts else None, _p(cns) if want_counts else None))
    return (rates, iters, ll, flags, csh, cns) if want_counts else (rates, iters, ll, flags)


def bootstrap_em_batch_groups(age_grid_, ages, weights, tables, epochs, init_rates=None, max_iter=DEFAULT_MAX_ITER,
                              min_iter=DEFAULT_MIN_ITER, rel_tol=DEFAULT_REL_TOL, rate_floor=DEFAULT_RATE_FLOOR,
                              want_counts=False):
    """colate_bootstrap_em_batch_groups (batched all-pairs): per group g a sample age ages[g], weights[g] = [B][nb_g],
    tables[g] = (sh, ns, sh_emp, ns_emp) each [nb_g][A], epochs[g] = [E].  Row g * B + i of the outputs = replicate i
    of group g."""
    return _bootstrap_em_batch_groups(None, age_grid_, ages, weights, tables, epochs, init_rates, max_iter, min_iter, rel_tol,
                                      rate_floor, want_counts)


def bootstrap_em_batch_groups_sharded(devices, age_grid_, ages, weights, tables, epochs, init_rates=None,
                                      max_iter=DEFAULT_MAX_ITER, min_iter=DEFAULT_MIN_ITER, rel_tol=DEFAULT_REL_TOL,
                                      rate_floor=DEFAULT_RATE_FLOOR, want_counts=False):
    """colate_bootstrap_em_batch_groups_sharded: bootstrap_em_batch_groups with the G * B rows sharded over the GPUs listed
    in `devices` (ordinals may repeat; a shard may begin and end inside a group)."""
    return _bootstrap_em_batch_groups(devices, age_grid_, ages, weights, tables, epochs, init_rates, max_iter, min_iter,
                                      rel_tol, rate_floor, want_counts)


def bootstrap_counts_groups_device(G, B, group_first, row_lo, row_hi, age_grid_, group_nb, group_block_off, group_weight_off, group_age,
                                   weights, sh_block, ns_block, sh_emp_block, ns_emp_block, cnt_shared, cnt_notshared, status, stream=None):
    """colate_bootstrap_counts_groups_device on torch tensors in HBM: the block bootstrap of rows [row_lo, row_hi) of G groups x B
    replicates (group arrays from group `group_first` on: int32 nb, int64 block / weight offsets, float64 ages); asynchronous."""
    A = age_grid_.numel()
    for t in (age_grid_, group_nb, group_block_off, group_weight_off, group_age, weights, sh_block, ns_block, sh_emp_block, ns_emp_block,
              cnt_shared, cnt_notshared, status):
        assert t.is_cuda and t.is_contiguous()
    check(lib.colate_bootstrap_counts_groups_device(int(G), int(B), int(group_first), int(row_lo), int(row_hi), A, age_grid_.data_ptr(),
                                                    group_nb.data_ptr(), group_block_off.data_ptr(), group_weight_off.data_ptr(),
                                                    group_age.data_ptr(), weights.data_ptr(), sh_block.data_ptr(), ns_block.data_ptr(),
                                                    sh_emp_block.data_ptr(), ns_emp_block.data_ptr(), cnt_shared.data_ptr(),
                                                    cnt_notshared.data_ptr(), status.data_ptr(), _stream_ptr(stream)))


def write_coal(path, epochs, rates, is_ancient=False, ep_null=0):
    e = _f64(epochs)
    r = _f64(np.atleast_2d(rates))
    check(lib.colate_write_coal(str(path).encode(), r.shape[0], e.size, _p(e), _p(r), int(is_ancient), ep_null))


def mut_main(argv):
    """The `Colate --mode mut ...` command line (argv without the program name)."""
    args = [b"Colate"] + [str(a).encode() for a in argv]
    arr = (c_char_p * len(args))(*args)
    return lib.colate_mut_main(len(args), arr)


def em_batch(age_grid_, cnt_shared, cnt_notshared, epochs, init_rates=None, max_iter=DEFAULT_MAX_ITER,
             min_iter=DEFAULT_MIN_ITER, rel_tol=DEFAULT_REL_TOL, rate_floor=DEFAULT_RATE_FLOOR):
    """colate_em_batch on host arrays.  Returns (rates[B][E], iters[B], loglik[B], flags[B])."""
    g, sh, ns, ep = _f64(age_grid_), _f64(np.atleast_2d(cnt_shared)), _f64(np.atleast_2d(cnt_notshared)), _f64(epochs)
    B, A = sh.shape
    E = ep.size
    init = _f64(np.full(E, DEFAULT_INIT_RATE) if init_rates is None else init_rates)
    rates = np.zeros((B, E))
    iters = np.zeros(B, dtype=np.int32)
    ll = np.zeros(B)
    flags = np.zeros(B, dtype=np.int32)
    check(lib.colate_em_batch(B, E, A, _p(g), _p(sh), _p(ns), _p(ep), _p(init), max_iter, min_iter, rel_tol,
                              rate_floor, _p(rates), _p(iters), _p(ll), _p(flags)))
    return rates, iters, ll, flags


def em_batch_rows(age_grid_, cnt_shared, cnt_notshared, epochs_rows, init_rows=None, max_iter=DEFAULT_MAX_ITER,
                  min_iter=DEFAULT_MIN_ITER, rel_tol=DEFAULT_REL_TOL, rate_floor=DEFAULT_RATE_FLOOR):
    """colate_em_batch_rows: epochs[B][E] (and starting rates) per replicate -- batched all-pairs."""
    g, sh, ns, ep = _f64(age_grid_), _f64(np.atleast_2d(cnt_shared)), _f64(np.atleast_2d(cnt_notshared)), _f64(epochs_rows)
    B, A = sh.shape
    E = ep.shape[1]
    assert ep.shape == (B, E)
    init = _f64(np.full((B, E), DEFAULT_INIT_RATE) if init_rows is None else init_rows)
    rates = np.zeros((B, E))
    iters = np.zeros(B, dtype=np.int32)
    ll = np.zeros(B)
    flags = np.zeros(B, dtype=np.int32)
    check(lib.colate_em_batch_rows(B, E, A, _p(g), _p(sh), _p(ns), _p(ep), _p(init), max_iter, min_iter, rel_tol,
                                   rate_floor, _p(rates), _p(iters), _p(ll), _p(flags)))
    return rates, iters, ll, flags


def em_batch_sharded(devices, age_grid_, cnt_shared, cnt_notshared, epochs, init_rates=None, max_iter=DEFAULT_MAX_ITER,
                     min_iter=DEFAULT_MIN_ITER, rel_tol=DEFAULT_REL_TOL, rate_floor=DEFAULT_RATE_FLOOR):
    """colate_em_batch_sharded: one process drives the GPUs listed in `devices` (ordinals may repeat)."""
    g, sh, ns, ep = _f64(age_grid_), _f64(np.atleast_2d(cnt_shared)), _f64(np.atleast_2d(cnt_notshared)), _f64(epochs)
    B, A = sh.shape
    E = ep.size
    init = _f64(np.full(E, DEFAULT_INIT_RATE) if init_rates is None else init_rates)
    dev = np.ascontiguousarray(devices, dtype=np.int32)
    rates = np.zeros((B, E))
    iters = np.zeros(B, dtype=np.int32)
    ll = np.zeros(B)
    flags = np.zeros(B, dtype=np.int32)
    check(lib.colate_em_batch_sharded(dev.size, _p(dev), B, E, A, _p(g), _p(sh), _p(ns), _p(ep), _p(init), max_iter,
                                      min_iter, rel_tol, rate_floor, _p(rates), _p(iters), _p(ll), _p(flags)))
    return rates, iters, ll, flags


def em_batch_rows_sharded(devices, age_grid_, cnt_shared, cnt_notshared, epochs, init_rates=None,
                          max_iter=DEFAULT_MAX_ITER, min_iter=DEFAULT_MIN_ITER, rel_tol=DEFAULT_REL_TOL,
                          rate_floor=DEFAULT_RATE_FLOOR):
    """colate_em_batch_rows_sharded: per-row epochs[B][E] (batched pairs), rows sharded over `devices`."""
    g, sh, ns = _f64(age_grid_), _f64(np.atleast_2d(cnt_shared)), _f64(np.atleast_2d(cnt_notshared))
    ep = _f64(np.atleast_2d(epochs))
    B, A = sh.shape
    E = ep.shape[1]
    assert ep.shape == (B, E)
    init = _f64(np.full((B, E), DEFAULT_INIT_RATE) if init_rates is None else np.atleast_2d(init_rates))
    assert init.shape == (B, E)
    dev = np.ascontiguousarray(devices, dtype=np.int32)
    rates = np.zeros((B, E))
    iters = np.zeros(B, dtype=np.int32)
    ll = np.zeros(B)
    flags = np.zeros(B, dtype=np.int32)
    check(lib.colate_em_batch_rows_sharded(dev.size, _p(dev), B, E, A, _p(g), _p(sh), _p(ns), _p(ep), _p(init), max_iter,
                                           min_iter, rel_tol, rate_floor, _p(rates), _p(iters), _p(ll), _p(flags)))
    return rates, iters, ll, flags


def em_estep(age_grid_, cnt_shared, cnt_notshared, epochs, rates):
    """colate_em_estep on host arrays: rates[B][E] -> (num[B][E], den[B][E], loglik[B], flags[B])."""
    g, sh, ns, ep = _f64(age_grid_), _f64(np.atleast_2d(cnt_shared)), _f64(np.atleast_2d(cnt_notshared)), _f64(epochs)
    r = _f64(np.atleast_2d(rates))
    B, A = sh.shape
    E = ep.size
    assert r.shape == (B, E)
    num = np.zeros((B, E))
    den = np.zeros((B, E))
    ll = np.zeros(B)
    flags = np.zeros(B, dtype=np.int32)
    check(lib.colate_em_estep(B, E, A, _p(g), _p(sh), _p(ns), _p(ep), _p(r), _p(num), _p(den), _p(ll), _p(flags)))
    return num, den, ll, flags


def em_interval_calls(kinds, age_begin, age_end, epochs, rates, weights=None, device=True, math=1):
    """colate_em_interval_calls: coal_EM::EM_shared (kind 0) / EM_notshared (kind 1) for R calls (age_begin[r], age_end[r])
    against one (epochs[E], rates[E]) -- interval-dated mutations, age uniform on [age_begin, age_end]; rows with equal ages
    are the point form.  Returns (num[R][E], den[R][E], logl[R], flags[R]) and, with weights[R], also (num_acc[E],
    den_acc[E], ll): the calls summed as one E-step, rows in ascending order.  device=False: the host twins
    (colate_em_interval_calls_host; math 0 = <cmath>, bit for bit the reference; math 1 = em_math, bit for bit the device)."""
    k = np.ascontiguousarray(np.atleast_1d(kinds), dtype=np.int32)
    a0, a1, ep, r = _f64(np.atleast_1d(age_begin)), _f64(np.atleast_1d(age_end)), _f64(epochs), _f64(rates)
    R, E = k.size, ep.size
    if a0.shape != (R,) or a1.shape != (R,) or r.shape != (E,):
        raise ValueError("kinds, age_begin, age_end must have one entry per call and rates one per epoch")
    w = None if weights is None else _f64(np.atleast_1d(weights))
    if w is not None and w.shape != (R,):
        raise ValueError("weights must have one entry per call")
    num, den, ll, flags = np.zeros((R, E)), np.zeros((R, E)), np.zeros(R), np.zeros(R, dtype=np.int32)
    nacc, dacc, lls = np.zeros(E), np.zeros(E), np.zeros(1)
    args = [R, E, _p(k), _p(a0), _p(a1), _p(ep), _p(r), None if w is None else _p(w), _p(num), _p(den), _p(ll), _p(flags),
            None if w is None else _p(nacc), None if w is None else _p(dacc), None if w is None else _p(lls)]
    check(lib.colate_em_interval_calls(*args) if device else lib.colate_em_interval_calls_host(*args, int(math)))
    return (num, den, ll, flags) if w is None else (num, den, ll, flags, nacc, dacc, float(lls[0]))


def em_interval_batch(kinds, age_begin, age_end, weights, epochs, init_rates=None, max_iter=DEFAULT_MAX_ITER,
                      min_iter=DEFAULT_MIN_ITER, rel_tol=DEFAULT_REL_TOL, rate_floor=DEFAULT_RATE_FLOOR, device=True, math=1):
    """colate_em_interval_batch: the EM fit on interval-dated mutations.  R rows (kinds[r], age_begin[r], age_end[r]) shared by
    B replicates, weights[B][R] (1-D: B = 1) the bootstrap-weighted count of row r in replicate b; M-step, floor and stop
    rule as in em_batch.  Returns (rates[B][E], iters[B], loglik[B], flags[B]).  device=False: the host twins
    (colate_em_interval_batch_host; math 0 = <cmath>, bit for bit the reference's loop; math 1 = em_math, bit for bit the device)."""
    k = np.ascontiguousarray(np.atleast_1d(kinds), dtype=np.int32)
    a0, a1, ep = _f64(np.atleast_1d(age_begin)), _f64(np.atleast_1d(age_end)), _f64(epochs)
    w = _f64(np.atleast_2d(weights))
    R, E, B = k.size, ep.size, w.shape[0]
    if a0.shape != (R,) or a1.shape != (R,) or w.shape != (B, R):
        raise ValueError("kinds, age_begin, age_end must have one entry per row and weights one row of them per replicate")
    init = _f64(np.full(E, DEFAULT_INIT_RATE) if init_rates is None else init_rates)
    if init.shape != (E,):
        raise ValueError("init_rates must have one entry per epoch")
    rates, iters, ll, flags = np.zeros((B, E)), np.zeros(B, dtype=np.int32), np.zeros(B), np.zeros(B, dtype=np.int32)
    args = [B, R, E, _p(k), _p(a0), _p(a1), _p(w), _p(ep), _p(init), int(max_iter), int(min_iter), float(rel_tol),
            float(rate_floor), _p(rates), _p(iters), _p(ll), _p(flags)]
    check(lib.colate_em_interval_batch(*args) if device else lib.colate_em_interval_batch_host(*args, int(math)))
    return rates, iters, ll, flags


def bootstrap_rows(block_weights, tables):
    """colate_bootstrap_rows_host: W[B][R] = block_weights[B][nb] x tables[nb][R], per element summed from 0.0 over the blocks
    in ascending order, every product rounded and then added -- the host twin of the bootstrap kernel in front of the
    interval-dated fit (bit for bit its sums)."""
    bw, t = _f64(np.atleast_2d(block_weights)), _f64(np.atleast_2d(tables))
    if bw.ndim != 2 or t.ndim != 2 or bw.shape[1] != t.shape[0]:
        raise ValueError("block_weights must be [B][nb] and tables [nb][R]")
    W = np.zeros((bw.shape[0], t.shape[1]))
    check(lib.colate_bootstrap_rows_host(bw.shape[0], t.shape[0], t.shape[1], _p(bw), _p(t), _p(W)))
    return W


def bootstrap_em_interval_batch(kinds, age_begin, age_end, block_weights, tables, epochs, init_rates=None,
                                max_iter=DEFAULT_MAX_ITER, min_iter=DEFAULT_MIN_ITER, rel_tol=DEFAULT_REL_TOL,
                                rate_floor=DEFAULT_RATE_FLOOR, device=True, math=1):
    """colate_bootstrap_em_interval_batch: the block bootstrap and the EM fit on interval-dated mutations in one call.
    tables[nb][R] holds per genome block the weights of the R rows (kinds[r], age_begin[r], age_end[r]), block_weights[B][nb]
    (1-D: B = 1) the replicates' block weights (bootstrap_weights); the fit runs on bootstrap_rows(block_weights, tables),
    which on the device never leaves it.  Returns (rates[B][E], iters[B], loglik[B], flags[B]) -- em_interval_batch's on that
    W, bit for bit.  device=False: the host twin (colate_bootstrap_em_interval_batch_host; math as for em_interval_batch)."""
    k = np.ascontiguousarray(np.atleast_1d(kinds), dtype=np.int32)
    a0, a1, ep = _f64(np.atleast_1d(age_begin)), _f64(np.atleast_1d(age_end)), _f64(epochs)
    bw, t = _f64(np.atleast_2d(block_weights)), _f64(np.atleast_2d(tables))
    R, E, B, nb = k.size, ep.size, bw.shape[0], t.shape[0]
    if a0.shape != (R,) or a1.shape != (R,) or t.shape != (nb, R) or bw.shape != (B, nb):
        raise ValueError("kinds, age_begin, age_end must have one entry per row, tables one row of them per block and "
                         "block_weights one weight per block and replicate")
    init = _f64(np.full(E, DEFAULT_INIT_RATE) if init_rates is None else init_rates)
    if init.shape != (E,):
        raise ValueError("init_rates must have one entry per epoch")
    rates, iters, ll, flags = np.zeros((B, E)), np.zeros(B, dtype=np.int32), np.zeros(B), np.zeros(B, dtype=np.int32)
    args = [B, nb, R, E, _p(k), _p(a0), _p(a1), _p(bw), _p(t), _p(ep), _p(init), int(max_iter), int(min_iter), float(rel_tol),
            float(rate_floor), _p(rates), _p(iters), _p(ll), _p(flags)]
    check(lib.colate_bootstrap_em_interval_batch(*args) if device else lib.colate_bootstrap_em_interval_batch_host(*args, int(math)))
    return rates, iters, ll, flags


def em_interval_batch_waves(E):
    """How many rows a workgroup of em_interval_batch calls at a time for E epochs."""
    return lib.colate_em_interval_batch_waves(int(E))


INTERVAL_BINS = 185
INTERVAL_MAX_ROWS = INTERVAL_BINS * (INTERVAL_BINS + 1)
INTERVAL_REC = np.dtype([("begin", np.float32), ("end", np.float32), ("w_sh", np.float64), ("w_ns", np.float64)])


def interval_bin_thresholds():
    """float32 [185]: entry n - 1 is the smallest float whose age bin (coal.cpp:2265 on the float widened to double) is
    >= n, so that the bin of x is the number of entries <= x (colate_interval_bin_thresholds)."""
    T = np.zeros(INTERVAL_BINS, dtype=np.float32)
    check(lib.colate_interval_bin_thresholds(_p(T)))
    return T


def interval_cells_tile():
    """Cells of the (bb, be) triangle per tile of the interval-cells kernel (diagnostic; no device needed)."""
    return lib.colate_interval_cells_tile()


def interval_cells(begin, end, w_sh, w_ns, block, nb, device=True, max_rows=None):
    """The used SNPs of a pair -- float32 ages begin <= end, weights w_sh / w_ns, genome block per record (not decreasing,
    in [0, nb)) -- as the rows and per-block tables of bootstrap_em_interval_batch (colate_interval_cells[_host]): ages
    snapped to the age grid, per (block, kind, bin(begin), bin(end)) the weights summed from 0.0 in record order.
    Returns (kinds [R], age_begin [R], age_end [R], tables [nb, R], dropped): the rows with a positive sum in at least one
    block, ordered by kind, bin(begin), bin(end); dropped = records beyond the age grid.  device=False: the host twin
    (the same doubles).  max_rows: the room given (default: always enough)."""
    recs = np.zeros(np.asarray(begin).size, dtype=INTERVAL_REC)
    recs["begin"], recs["end"], recs["w_sh"], recs["w_ns"] = np.ravel(begin), np.ravel(end), np.ravel(w_sh), np.ravel(w_ns)
    block = np.ascontiguousarray(block, dtype=np.int32).ravel()
    if block.size != recs.size:
        raise ValueError("one block index per record")
    nb = int(nb)
    cap = min(INTERVAL_MAX_ROWS, 2 * recs.size) if max_rows is None else int(max_rows)
    kinds = np.zeros(cap, dtype=np.int32)
    a0, a1 = np.zeros(cap), np.zeros(cap)
    tables = np.zeros(max(nb, 0) * cap)
    dropped = ctypes.c_longlong(0)
    fn = lib.colate_interval_cells if device else lib.colate_interval_cells_host
    R = check(fn(recs.size, _p(recs), _p(block), nb, cap, _p(kinds), _p(a0), _p(a1), _p(tables), ctypes.addressof(dropped)))
    return kinds[:R].copy(), a0[:R].copy(), a1[:R].copy(), tables[:nb * R].reshape(nb, R).copy(), int(dropped.value)


def interval_fit_groups(groups, epochs, init_rates=None, max_iter=DEFAULT_MAX_ITER, min_iter=DEFAULT_MIN_ITER,
                        rel_tol=DEFAULT_REL_TOL, rate_floor=DEFAULT_RATE_FLOOR, device=True, math=1):
    """colate_interval_fit_groups: for each group -- a tuple (begin, end, w_sh, w_ns, block, nb, block_weights[B][nb]), the
    records as interval_cells takes them and the block weights of its B replicates -- interval_cells followed by
    bootstrap_em_interval_batch, all groups in one call; on the device neither the cell sums nor W leave it.  epochs and
    init_rates: [E] for all groups or [G][E].  Returns (R[G], dropped[G], rates[G][B][E], iters[G][B], loglik[G][B],
    flags[G][B]): per group, bit for bit, what the two single calls return; a group without rows keeps its starting rates,
    with iters, loglik and flags 0.  device=False: the host twin (colate_interval_fit_groups_host; math as for
    em_interval_batch)."""
    G = len(groups)
    recs, blocks, nbs, bws, rec_off = [], [], [], [], [0]
    B = None
    for begin, end, w_sh, w_ns, block, nb, block_weights in groups:
        r = np.zeros(np.asarray(begin).size, dtype=INTERVAL_REC)
        r["begin"], r["end"], r["w_sh"], r["w_ns"] = np.ravel(begin), np.ravel(end), np.ravel(w_sh), np.ravel(w_ns)
        blk = np.ascontiguousarray(block, dtype=np.int32).ravel()
        bw = _f64(np.atleast_2d(block_weights))
        if blk.size != r.size:
            raise ValueError("one block index per record")
        if bw.shape[1] != int(nb) or (B is not None and bw.shape[0] != B):
            raise ValueError("block_weights must be [B][nb] with the same B in every group")
        B = bw.shape[0]
        recs.append(r), blocks.append(blk), nbs.append(int(nb)), bws.append(bw.ravel())
        rec_off.append(rec_off[-1] + r.size)
    B = 0 if B is None else B
    ep = _f64(epochs)
    E = ep.shape[-1]
    ep = _f64(np.broadcast_to(ep, (G, E))) if ep.ndim == 1 else ep
    init = _f64(np.full(E, DEFAULT_INIT_RATE) if init_rates is None else init_rates)
    init = _f64(np.broadcast_to(init, (G, E))) if init.ndim == 1 else init
    if ep.shape != (G, E) or init.shape != (G, E):
        raise ValueError("epochs and init_rates must be [E] or [G][E]")
    recs = np.concatenate(recs) if G else np.zeros(0, dtype=INTERVAL_REC)
    blocks = np.ascontiguousarray(np.concatenate(blocks) if G else np.zeros(0), dtype=np.int32)
    bws = _f64(np.concatenate(bws) if G else np.zeros(0))
    rec_off, nbs = np.asarray(rec_off, dtype=np.int64), np.asarray(nbs, dtype=np.int32)
    R, dropped = np.zeros(G, dtype=np.int32), np.zeros(G, dtype=np.int64)
    rates, iters, ll, flags = np.zeros((G, B, E)), np.zeros((G, B), dtype=np.int32), np.zeros((G, B)), np.zeros((G, B), dtype=np.int32)
    args = [G, B, E, _p(rec_off), _p(recs), _p(blocks), _p(nbs), _p(bws), _p(ep), _p(init), int(max_iter), int(min_iter),
            float(rel_tol), float(rate_floor), _p(R), _p(dropped), _p(rates), _p(iters), _p(ll), _p(flags)]
    check(lib.colate_interval_fit_groups(*args) if device else lib.colate_interval_fit_groups_host(*args, int(math)))
    return R, dropped, rates, iters, ll, flags


WALK_ROW = np.dtype([("pos", np.int32), ("age_begin", np.float32), ("age_end", np.float32)])
WALK_IDX = np.dtype([("prev_bp", np.int32), ("DAF", np.uint16), ("AAF", np.uint16)])
WALK_PAIR = np.dtype([("target", np.int32), ("reference", np.int32), ("target_mask", np.int32), ("reference_mask", np.int32)])


def interval_walk_tile():
    """Rows of a chromosome a workgroup of the pair-walk kernel looks at per step (diagnostic; no device needed)."""
    return lib.colate_interval_walk_tile()


def _walk_inputs(row_off, rows, idx, masks, pairs):
    row_off = np.ascontiguousarray(row_off, dtype=np.int64).ravel()
    rows = np.ascontiguousarray(rows, dtype=WALK_ROW).ravel()
    idx = np.ascontiguousarray(idx, dtype=WALK_IDX)
    pairs = np.ascontiguousarray(pairs, dtype=WALK_PAIR).ravel()
    masks = np.zeros((0, 0), dtype=np.uint64) if masks is None else np.ascontiguousarray(masks, dtype=np.uint64)
    if idx.ndim != 2 or idx.shape[1] != rows.size:
        raise ValueError("idx must be [S][rows]")
    if masks.ndim != 2:
        raise ValueError("masks must be [M][words]")
    if row_off.size >= 2 and row_off[0] == 0 and (np.diff(row_off) >= 0).all():  # (else the library names what is wrong)
        if row_off[-1] != rows.size:
            raise ValueError("row_off[-1] must be the number of rows")
        if masks.shape[0] and masks.shape[1] != int(((np.diff(row_off) + 63) // 64).sum()):
            raise ValueError("a mask holds ceil(rows / 64) words per chromosome")
    return [row_off.size - 1, _p(row_off), _p(rows), idx.shape[0], _p(idx), masks.shape[0], _p(masks), pairs.size, _p(pairs)], \
        (row_off, rows, idx, masks, pairs)


def interval_walk(row_off, rows, idx, masks, pairs, num_bases_per_block, device=True, cap=None):
    """colate_interval_walk[_host]: the pair walk of `--mode mut_interval` for every pair of `pairs` over per-sample walk
    indices.  row_off [C + 1]: the chromosomes' rows back to back in rows (WALK_ROW); idx [S][rows] (WALK_IDX); masks
    [M][words] uint64 or None (one bit per row, each chromosome starting on a word); pairs (WALK_PAIR: sample ids, mask ids
    or -1).  Returns (rec_off [P + 1], nb [P], recs (INTERVAL_REC), block): every pair's used SNPs and their genome blocks
    back to back.  cap: the room given (default: every row of every pair).  device=False: the host twin, the same bytes."""
    args, keep = _walk_inputs(row_off, rows, idx, masks, pairs)
    P = keep[4].size
    cap = P * keep[1].size if cap is None else int(cap)
    rec_off, nb = np.zeros(P + 1, dtype=np.int64), np.zeros(P, dtype=np.int32)
    recs, block = np.zeros(max(cap, 0), dtype=INTERVAL_REC), np.zeros(max(cap, 0), dtype=np.int32)
    fn = lib.colate_interval_walk if device else lib.colate_interval_walk_host
    check(fn(*args, int(num_bases_per_block), cap, _p(rec_off), _p(nb), _p(recs), _p(block)))
    n = int(rec_off[-1])
    return rec_off, nb, recs[:n].copy(), block[:n].copy()


def interval_fit_samples(row_off, rows, idx, masks, pairs, num_bases_per_block, num_bootstrap, epochs, seed, init_rates=None,
                         max_iter=DEFAULT_MAX_ITER, min_iter=DEFAULT_MIN_ITER, rel_tol=DEFAULT_REL_TOL,
                         rate_floor=DEFAULT_RATE_FLOOR, device=True, math=1):
    """colate_interval_fit_samples[_host]: interval_walk followed by interval_fit_groups on its records (group p = pair p),
    the records never leaving the device; every pair's block weights [B][nb] are drawn by the call from a fresh mt19937 on
    `seed` (bootstrap_weights).  epochs / init_rates: [E] for all pairs.  Returns (nb[P], used[P], R[P], dropped[P],
    rates[P][B][E], iters[P][B], loglik[P][B], flags[P][B]).  device=False: the host twin (math as for em_interval_batch)."""
    args, keep = _walk_inputs(row_off, rows, idx, masks, pairs)
    P, B = keep[4].size, int(num_bootstrap)
    ep = _f64(epochs).ravel()
    E = ep.size
    init = _f64(np.full(E, DEFAULT_INIT_RATE) if init_rates is None else init_rates).ravel()
    if init.size != E:
        raise ValueError("init_rates must be [E]")
    Bn = max(B, 0)
    nb, used = np.zeros(P, dtype=np.int32), np.zeros(P, dtype=np.int64)
    R, dropped = np.zeros(P, dtype=np.int32), np.zeros(P, dtype=np.int64)
    rates, iters, ll, flags = np.zeros((P, Bn, E)), np.zeros((P, Bn), dtype=np.int32), np.zeros((P, Bn)), np.zeros((P, Bn), dtype=np.int32)
    full = args + [int(num_bases_per_block), B, E, _p(ep), _p(init), int(seed) & 0xffffffff, int(max_iter), int(min_iter),
                   float(rel_tol), float(rate_floor), _p(nb), _p(used), _p(R), _p(dropped), _p(rates), _p(iters), _p(ll), _p(flags)]
    check(lib.colate_interval_fit_samples(*full) if device else lib.colate_interval_fit_samples_host(*full, int(math)))
    return nb, used, R, dropped, rates, iters, ll, flags


def interval_fit_samples_kernel_seconds():
    """Seconds the kernels of this thread's last interval_fit_samples(device=True) took on the device, the walk included."""
    return lib.colate_interval_fit_samples_kernel_seconds()


def fill_samples(row_off, rows, idx, masks, pairs, num_bases_per_block, seed, A=185, device=True, cap_blocks=None):
    """colate_fill_samples[_host]: the table fill of `--mode mut` for every pair of `pairs` over per-sample walk indices (the
    inputs of interval_walk).  Returns a dict: nb [P], used [P], tables (a list of [nb[p]][4][A] arrays: shared, not shared,
    shared row 0, not-shared row 0 per block), words [P] (32-bit words each pair's mt19937 on `seed` has given out at the end
    of its fill), handed_back [P], and with device=False near_band [P] (None otherwise).  cap_blocks: the room given for
    tables (default: every block the positions allow).  device=False: the host twin, the same bytes."""
    args, keep = _walk_inputs(row_off, rows, idx, masks, pairs)
    row_off_, rows_ = keep[0], keep[1]
    P, A = keep[4].size, int(A)
    nbpb = int(num_bases_per_block)
    if cap_blocks is None:  # per chromosome at most the block of its last position, plus one
        cap_blocks = 0
        for c in range(row_off_.size - 1):
            seg = rows_["pos"][row_off_[c]:row_off_[c + 1]]
            cap_blocks += 1 + (max(int(seg.max()) - 1, 0) // max(nbpb, 1) if seg.size else 0)
        cap_blocks *= P
    cap_blocks = int(cap_blocks)
    nb, used = np.zeros(P, dtype=np.int32), np.zeros(P, dtype=np.int64)
    tables = np.zeros((max(cap_blocks, 0), 4, max(A, 0)))
    words, handed, near = np.zeros(P, dtype=np.uint64), np.zeros(P, dtype=np.int32), np.zeros(P, dtype=np.int32)
    full = args + [nbpb, A, int(seed) & 0xffffffff, cap_blocks, _p(nb), _p(used), _p(tables), _p(words), _p(handed)]
    check(lib.colate_fill_samples(*full) if device else lib.colate_fill_samples_host(*full, _p(near)))
    off = np.concatenate([[0], np.cumsum(nb)])
    return dict(nb=nb, used=used, tables=[tables[off[p]:off[p + 1]].copy() for p in range(P)], words=words, handed_back=handed,
                near_band=None if device else near)


def compare_samples(row_off, rows, idx, pairs, first_pos, last_pos, window, device=True, cap=None):
    """colate_compare_samples[_host]: the windowed pair mismatch of `--mode compare_tmp` for every pair of `pairs` over
    per-sample walk indices.  row_off, rows, idx, pairs: the inputs of interval_walk (no masks: a pair's mask ids are -1), every
    row a searched row; first_pos / last_pos [C]: the positions of each chromosome's first and last raw rows; window: the window
    in bases (the command line: 10 000 000).  Returns (win_off [C + 1], mismatch [P][win_off[C]], snps [P][win_off[C]]).  cap:
    the room given per output (default: what the call needs).  device=False: the host twin, the same ints."""
    args, keep = _walk_inputs(row_off, rows, idx, None, pairs)
    C, P = keep[0].size - 1, keep[4].size
    first_pos = np.ascontiguousarray(first_pos, dtype=np.int32).ravel()
    last_pos = np.ascontiguousarray(last_pos, dtype=np.int32).ravel()
    if first_pos.size != C or last_pos.size != C:
        raise ValueError("first_pos and last_pos hold one position per chromosome")
    window = int(window)
    if cap is None:  # (the library checks everything again and names what is wrong)
        f, l = first_pos.astype(np.int64), last_pos.astype(np.int64)
        cap = P * int((np.where(l > f, (l - f - 1) // max(window, 1), 0) + 1).sum())
    cap = int(cap)
    win_off = np.zeros(C + 1, dtype=np.int64)
    mismatch, snps = np.zeros(max(cap, 0), dtype=np.int32), np.zeros(max(cap, 0), dtype=np.int32)
    fn = lib.colate_compare_samples if device else lib.colate_compare_samples_host
    check(fn(args[0], args[1], args[2], args[3], args[4], args[7], args[8], _p(first_pos), _p(last_pos), window, cap, _p(win_off),
             _p(mismatch), _p(snps)))
    n = int(win_off[-1])
    return win_off, mismatch[:P * n].reshape(P, n).copy(), snps[:P * n].reshape(P, n).copy()


def compare_samples_chunks():
    """Chunks of pairs in this thread's last compare_samples(device=True) (diagnostic)."""
    return lib.colate_compare_samples_chunks()


def compare_samples_kernel_seconds():
    """Seconds the kernels of this thread's last compare_samples(device=True) took on the device."""
    return lib.colate_compare_samples_kernel_seconds()


TOPO_TRIPLE = np.dtype([("cond", np.int32), ("target", np.int32), ("reference", np.int32)])


def topo_samples(row_off, rows, idx, cond_idx, triples, uniforms, device=True, cap=None):
    """colate_topo_samples[_host]: the signed topology counts of `--mode count_topo` for every (cond, target, reference) of
    `triples` (TOPO_TRIPLE: sample ids) over per-sample walk indices.  row_off, rows, idx: the inputs of interval_walk, every row
    a searched row of this mode; cond_idx [S][rows] (WALK_IDX): per sample and row the counts of the record its cursor stands on,
    matched or not; uniforms: the stream every triple reads from its start, two per qualifying row.  Returns (word_off [C + 1],
    plus [P][words] uint64, minus [P][words], draws [P]): bit i & 63 of word word_off[c] + (i >> 6) is row i of chromosome c.
    cap: the room given per plane in words (default: what the call needs).  device=False: the host twin, the same bits."""
    args, keep = _walk_inputs(row_off, rows, idx, None, np.zeros(0, dtype=WALK_PAIR))
    row_off_ = keep[0]
    cond_idx = np.ascontiguousarray(cond_idx, dtype=WALK_IDX)
    if cond_idx.shape != keep[2].shape:
        raise ValueError("cond_idx must be [S][rows], as idx")
    triples = np.ascontiguousarray(triples, dtype=TOPO_TRIPLE).ravel()
    uniforms = _f64(uniforms).ravel()
    P = triples.size
    words = int(((np.diff(row_off_) + 63) // 64).sum()) if row_off_.size >= 2 and (np.diff(row_off_) >= 0).all() else 0
    cap = P * words if cap is None else int(cap)  # (the library checks everything again and names what is wrong)
    word_off, draws = np.zeros(row_off_.size, dtype=np.int64), np.zeros(P, dtype=np.int64)
    plus, minus = np.zeros(max(cap, 0), dtype=np.uint64), np.zeros(max(cap, 0), dtype=np.uint64)
    fn = lib.colate_topo_samples if device else lib.colate_topo_samples_host
    check(fn(args[0], args[1], args[2], args[3], args[4], _p(cond_idx), P, _p(triples), uniforms.size, _p(uniforms), cap, _p(word_off),
             _p(plus), _p(minus), _p(draws)))
    n = int(word_off[-1])
    return word_off, plus[:P * n].reshape(P, n).copy(), minus[:P * n].reshape(P, n).copy(), draws


def topo_samples_tile():
    """Rows of a tile of the draw kernel of topo_samples: 64 words of 64 rows (no device needed)."""
    return lib.colate_topo_samples_tile()


def topo_samples_chunks():
    """Chunks of triples in this thread's last topo_samples(device=True) (diagnostic)."""
    return lib.colate_topo_samples_chunks()


def topo_samples_kernel_seconds():
    """Seconds the kernels of this thread's last topo_samples(device=True) took on the device."""
    return lib.colate_topo_samples_kernel_seconds()


def topo_profile(row_off, rows, idx, cond_idx, triples, uniforms, epochs, device=True):
    """colate_topo_profile[_host]: the draws of topo_samples counted per epoch, without a plane leaving the call.  Inputs as for
    topo_samples; epochs [E]: finite, strictly ascending, 1 <= E <= 1024.  A row's epoch is the number of e in 1 .. E - 1 with
    epochs[e] <= 0.5f * (age_begin + age_end), the mid formed in float32.  Returns (counts [P, E, 3] int64 -- plus, minus,
    qualifying --, draws [P] int64).  device=False: the host twin, the same integers."""
    args, keep = _walk_inputs(row_off, rows, idx, None, np.zeros(0, dtype=WALK_PAIR))
    cond_idx = np.ascontiguousarray(cond_idx, dtype=WALK_IDX)
    if cond_idx.shape != keep[2].shape:
        raise ValueError("cond_idx must be [S][rows], as idx")
    triples = np.ascontiguousarray(triples, dtype=TOPO_TRIPLE).ravel()
    uniforms = _f64(uniforms).ravel()
    epochs = _f64(epochs).ravel()
    P, E = triples.size, epochs.size
    counts, draws = np.zeros((P, E, 3), dtype=np.int64), np.zeros(P, dtype=np.int64)
    fn = lib.colate_topo_profile if device else lib.colate_topo_profile_host
    check(fn(args[0], args[1], args[2], args[3], args[4], _p(cond_idx), P, _p(triples), uniforms.size, _p(uniforms), E, _p(epochs),
             _p(counts), _p(draws)))
    return counts, draws


def topo_profile_chunks():
    """Chunks of triples in this thread's last topo_profile(device=True) (diagnostic)."""
    return lib.colate_topo_profile_chunks()


def topo_profile_kernel_seconds():
    """Seconds the kernels of this thread's last topo_profile(device=True) took on the device."""
    return lib.colate_topo_profile_kernel_seconds()


def topo_blocks(row_off, rows, num_bases_per_block):
    """colate_topo_blocks: blk_off [C + 1] int32 of the searched rows (no device needed).  With k(pos) = (pos - 1) //
    num_bases_per_block for pos > 0, else 0, a chromosome owns k(pos of its last row) + 1 blocks, or 1 without a row; a row's global
    block is blk_off[c] + k(pos).  A function of the rows alone: not the blocks of `--mode mut`."""
    row_off = np.ascontiguousarray(row_off, dtype=np.int64).ravel()
    rows = np.ascontiguousarray(rows, dtype=WALK_ROW).ravel()
    if row_off.size >= 2 and row_off[0] == 0 and (np.diff(row_off) >= 0).all() and row_off[-1] != rows.size:
        raise ValueError("row_off[-1] must be the number of rows")  # (else the library names what is wrong)
    blk_off = np.zeros(max(row_off.size, 1), dtype=np.int32)
    check(lib.colate_topo_blocks(row_off.size - 1, _p(row_off), _p(rows), int(num_bases_per_block), _p(blk_off)))
    return blk_off


def topo_profile_blocks(row_off, rows, idx, cond_idx, triples, uniforms, epochs, num_bases_per_block, device=True):
    """colate_topo_profile_blocks[_host]: topo_profile per genome block of topo_blocks, from the same draws.  Returns (blk_off
    [C + 1] int32, counts [P, nb, E, 3] int64 -- plus, minus, qualifying --, draws [P] int64); counts.sum(axis=1) is topo_profile's
    counts for every num_bases_per_block.  device=False: the host twin, the same integers."""
    blk_off = topo_blocks(row_off, rows, num_bases_per_block)
    args, keep = _walk_inputs(row_off, rows, idx, None, np.zeros(0, dtype=WALK_PAIR))
    cond_idx = np.ascontiguousarray(cond_idx, dtype=WALK_IDX)
    if cond_idx.shape != keep[2].shape:
        raise ValueError("cond_idx must be [S][rows], as idx")
    triples = np.ascontiguousarray(triples, dtype=TOPO_TRIPLE).ravel()
    uniforms = _f64(uniforms).ravel()
    epochs = _f64(epochs).ravel()
    P, E, nb = triples.size, epochs.size, int(blk_off[-1])
    counts, draws = np.zeros((P, nb, E, 3), dtype=np.int64), np.zeros(P, dtype=np.int64)
    fn = lib.colate_topo_profile_blocks if device else lib.colate_topo_profile_blocks_host
    check(fn(args[0], args[1], args[2], args[3], args[4], _p(cond_idx), P, _p(triples), uniforms.size, _p(uniforms), E, _p(epochs),
             int(num_bases_per_block), nb, _p(counts), _p(draws)))
    return blk_off, counts, draws


def topo_profile_blocks_chunks():
    """Chunks of triples in this thread's last topo_profile_blocks(device=True) (diagnostic)."""
    return lib.colate_topo_profile_blocks_chunks()


def topo_profile_blocks_kernel_seconds():
    """Seconds the kernels of this thread's last topo_profile_blocks(device=True) took on the device."""
    return lib.colate_topo_profile_blocks_kernel_seconds()


def topo_jackknife(counts):
    """colate_topo_jackknife: the weighted delete-one block jackknife (Busing, Meijer and van der Leeden) on one triple's counts
    [nb, E, 3] of topo_profile_blocks.  Returns (stats [E + 1, 4] float64 -- D, D_jack, se, Z per epoch and, last, for the sum over
    the epochs; NaN: not available --, used [E + 1] int32: the blocks with plus + minus > 0).  Host only."""
    counts = np.ascontiguousarray(counts, dtype=np.int64)
    if counts.ndim != 3 or counts.shape[2] != 3:
        raise ValueError("counts must be [nb][E][3], one triple's")
    nb, E = counts.shape[:2]
    stats, used = np.zeros((E + 1, 4), dtype=np.float64), np.zeros(E + 1, dtype=np.int32)
    check(lib.colate_topo_jackknife(nb, E, _p(counts), _p(stats), _p(used)))
    return stats, used


def topo_expected_blocks(row_off, rows, idx, cond_idx, triples, epochs, num_bases_per_block, device=True):
    """colate_topo_expected_blocks[_host]: what the draws of topo_profile_blocks estimate, formed without a draw.  At every
    qualifying row floor(DAF_T * AAF_R * 2^30 / (N_T * N_R)) goes to plus and floor(AAF_T * DAF_R * 2^30 / (N_T * N_R)) to minus:
    pT (1 - pR) and (1 - pT) pR in units of 2^-30, each short of the exact product by less than 2^-30.  Returns (blk_off [C + 1]
    int32, counts [P, nb, E, 3] int64 -- sum plus, sum minus, qualifying rows); counts[..., 2] is that of topo_profile_blocks, and
    topo_jackknife takes counts[p] as it is.  No uniforms, no seed.  device=False: the host twin, the same integers."""
    blk_off = topo_blocks(row_off, rows, num_bases_per_block)
    args, keep = _walk_inputs(row_off, rows, idx, None, np.zeros(0, dtype=WALK_PAIR))
    cond_idx = np.ascontiguousarray(cond_idx, dtype=WALK_IDX)
    if cond_idx.shape != keep[2].shape:
        raise ValueError("cond_idx must be [S][rows], as idx")
    triples = np.ascontiguousarray(triples, dtype=TOPO_TRIPLE).ravel()
    epochs = _f64(epochs).ravel()
    P, E, nb = triples.size, epochs.size, int(blk_off[-1])
    counts = np.zeros((P, nb, E, 3), dtype=np.int64)
    fn = lib.colate_topo_expected_blocks if device else lib.colate_topo_expected_blocks_host
    check(fn(args[0], args[1], args[2], args[3], args[4], _p(cond_idx), P, _p(triples), E, _p(epochs), int(num_bases_per_block), nb, _p(counts)))
    return blk_off, counts


def topo_expected_blocks_chunks():
    """Chunks of triples in this thread's last topo_expected_blocks(device=True) (diagnostic)."""
    return lib.colate_topo_expected_blocks_chunks()


def topo_expected_blocks_kernel_seconds():
    """Seconds the kernels of this thread's last topo_expected_blocks(device=True) took on the device."""
    return lib.colate_topo_expected_blocks_kernel_seconds()


def fill_samples_chunks():
    """Chunks of the write pass in this thread's last fill_samples(device=True) (diagnostic)."""
    return lib.colate_fill_samples_chunks()


def fill_samples_kernel_seconds():
    """Seconds the kernels of this thread's last fill_samples(device=True) took on the device."""
    return lib.colate_fill_samples_kernel_seconds()


def _stream_ptr(stream):
    if stream is None:
        import torch

        stream = torch.cuda.current_stream()
    return ctypes.c_void_p(stream.cuda_stream)


def em_batch_device(age_grid_, cnt_shared, cnt_notshared, epochs, init_rates, out_rates, out_iters, out_loglik,
                    out_flags, max_iter=DEFAULT_MAX_ITER, min_iter=DEFAULT_MIN_ITER, rel_tol=DEFAULT_REL_TOL,
                    rate_floor=DEFAULT_RATE_FLOOR, stream=None):
    """colate_em_batch_device on torch tensors resident in HBM (float64 / int32, contiguous).
    Asynchronous on `stream` (default: torch's current stream)."""
    B, A = cnt_shared.shape
    E = epochs.shape[-1]
    for t in (age_grid_, cnt_shared, cnt_notshared, epochs, init_rates, out_rates, out_iters, out_loglik, out_flags):
        assert t.is_cuda and t.is_contiguous()
    check(lib.colate_em_batch_device(B, E, A, age_grid_.data_ptr(), cnt_shared.data_ptr(), cnt_notshared.data_ptr(),
                                     epochs.data_ptr(), int(epochs.dim() == 2), init_rates.data_ptr(),
                                     int(init_rates.dim() == 2), max_iter, min_iter, rel_tol, rate_floor,
                                     out_rates.data_ptr(), out_iters.data_ptr(), out_loglik.data_ptr(),
                                     out_flags.data_ptr(), _stream_ptr(stream)))


def em_estep_device(age_grid_, cnt_shared, cnt_notshared, epochs, rates, num_acc, den_acc, loglik, flags, stream=None):
    B, A = cnt_shared.shape
    E = epochs.shape[-1]
    for t in (age_grid_, cnt_shared, cnt_notshared, epochs, rates, num_acc, den_acc, loglik, flags):
        assert t.is_cuda and t.is_contiguous()
    check(lib.colate_em_estep_device(B, E, A, age_grid_.data_ptr(), cnt_shared.data_ptr(), cnt_notshared.data_ptr(),
                                     epochs.data_ptr(), rates.data_ptr(), num_acc.data_ptr(), den_acc.data_ptr(),
                                     loglik.data_ptr(), flags.data_ptr(), _stream_ptr(stream)))


class coal_EM:
    """Mirror of the reference's `class coal_EM` (include/coal/coal_EM.hpp:14-63) on top of the GPU
    E-step, so that parity tests read like include/test/test_aDNA.cpp: construct with (epochs, rates),
    call EM_shared / EM_notshared(age_begin, age_end, num, denom) -> log-normaliser.

    age_begin == age_end -- the only way mut() calls it (coal.cpp:3708, 3721) -- is one E-step over a one-bin
    age grid with count 1, so num/denom/logl are exactly the reference's per-bin outputs; `EM_many` evaluates a
    whole list of ages in one launch.  age_begin < age_end (a mutation dated uniformly on its branch,
    coal_EM.cpp:212-242, 359-433) is one call of `em_interval_calls`, which takes whole batches of them."""

    def __init__(self, epochs, coal):
        self.epochs = _f64(epochs).copy()
        self.coal_rates = _f64(coal).copy()

    def UpdateCoal(self, coal):
        self.coal_rates = _f64(coal).copy()

    def EM_many(self, ages, shared):
        ages = _f64(np.atleast_1d(ages))
        n = ages.size
        # replicate i sees only age i: grid = all ages (sorted), count 1 at its own bin
        order = np.argsort(ages, kind="stable")
        grid = ages[order]
        cnt = np.zeros((n, n))
        cnt[np.arange(n), np.argsort(order, kind="stable")] = 1.0
        zero = np.zeros((n, n))
        rates = np.tile(self.coal_rates, (n, 1))
        sh, ns = (cnt, zero) if shared else (zero, cnt)
        num, den, ll, flags = em_estep(grid, sh, ns, self.epochs, rates)
        return num, den, ll, flags

    def _one(self, age_begin, age_end, num, denom, shared):
        if age_begin != age_end:
            n, d, ll, _ = em_interval_calls([0 if shared else 1], [age_begin], [age_end], self.epochs, self.coal_rates)
        else:
            n, d, ll, _ = self.EM_many([age_begin], shared)
        num[:] = n[0]
        denom[:] = d[0]
        return float(ll[0])

    def EM_shared(self, age_begin, age_end, num, denom):
        return self._one(age_begin, age_end, num, denom, True)

    def EM_notshared(self, age_begin, age_end, num, denom):
        return self._one(age_begin, age_end, num, denom, False)


def condcoal_accumulate(parents, branch_lengths, factors, blocks, num_blocks, group_of_hap, num_groups, focal, cond,
                        epochs, epochs_focal, sample_ages=None, device=True):
    """`--mode CondCoalRates` per-block accumulators (colate_condcoal_accumulate[_host]): parents / branch_lengths [T, 2N-1]
    (Relate labelling, root 2N-2), factors [T] (float32 tree weights), blocks [T]; group_of_hap [N]; focal / cond haplotype
    lists (cond empty: the empty conditional group); epochs / epochs_focal float32; sample_ages [N] or None.
    Returns (num, denom), float64 [num_blocks, EF, E, G].  device=False: the host twin."""
    parents = np.ascontiguousarray(parents, dtype=np.int32)
    T, nn = parents.shape if parents.ndim == 2 else (0, 1)
    N = (nn + 1) // 2
    if T == 0:
        N = len(group_of_hap)
    bl = _f64(branch_lengths).reshape(T, nn) if T else np.zeros((0, 1))
    factors = np.ascontiguousarray(factors, dtype=np.float32)
    blocks = np.ascontiguousarray(blocks, dtype=np.int32)
    group_of_hap = np.ascontiguousarray(group_of_hap, dtype=np.int32)
    focal = np.ascontiguousarray(focal, dtype=np.int32)
    cond = np.ascontiguousarray(cond, dtype=np.int32)
    epochs = np.ascontiguousarray(epochs, dtype=np.float32)
    epochs_focal = np.ascontiguousarray(epochs_focal, dtype=np.float32)
    ages = None if sample_ages is None else _f64(sample_ages)
    E, EF, G = epochs.size, epochs_focal.size, int(num_groups)
    num = np.zeros((int(num_blocks), EF, E, G))
    denom = np.zeros_like(num)
    fn = lib.colate_condcoal_accumulate if device else lib.colate_condcoal_accumulate_host
    check(fn(N, T, _p(parents), _p(bl), _p(factors), _p(blocks), int(num_blocks), G, _p(group_of_hap), focal.size, _p(focal),
             cond.size, _p(cond) if cond.size else None, _p(ages) if ages is not None else None, E, _p(epochs), EF,
             _p(epochs_focal), _p(num), _p(denom)))
    return num, denom


def condcoal_accumulate_pairs(parents, branch_lengths, factors, blocks, num_blocks, group_of_hap, num_groups, focal_group,
                              cond_group, epochs, epochs_focal, sample_ages=None, device=True):
    """condcoal_accumulate for many (focal group, conditional group) pairs in one pass over the trees
    (colate_condcoal_accumulate_pairs[_host]): focal_group / cond_group [P] group indices (cond_group -1: the empty
    conditional group; the focal haplotypes of a pair are all of its focal group's); blocks must not decrease.
    Returns (num, denom), float64 [P, num_blocks, EF, E, G]; pair p's part is bit for bit condcoal_accumulate's for it."""
    parents = np.ascontiguousarray(parents, dtype=np.int32)
    T, nn = parents.shape if parents.ndim == 2 else (0, 1)
    N = (nn + 1) // 2
    if T == 0:
        N = len(group_of_hap)
    bl = _f64(branch_lengths).reshape(T, nn) if T else np.zeros((0, 1))
    factors = np.ascontiguousarray(factors, dtype=np.float32)
    blocks = np.ascontiguousarray(blocks, dtype=np.int32)
    group_of_hap = np.ascontiguousarray(group_of_hap, dtype=np.int32)
    focal_group = np.ascontiguousarray(focal_group, dtype=np.int32).ravel()
    cond_group = np.ascontiguousarray(cond_group, dtype=np.int32).ravel()
    if focal_group.size != cond_group.size:
        raise ValueError("focal_group and cond_group differ in length")
    epochs = np.ascontiguousarray(epochs, dtype=np.float32)
    epochs_focal = np.ascontiguousarray(epochs_focal, dtype=np.float32)
    ages = None if sample_ages is None else _f64(sample_ages)
    E, EF, G, P = epochs.size, epochs_focal.size, int(num_groups), focal_group.size
    num = np.zeros((P, int(num_blocks), EF, E, G))
    denom = np.zeros_like(num)
    fn = lib.colate_condcoal_accumulate_pairs if device else lib.colate_condcoal_accumulate_pairs_host
    check(fn(N, T, _p(parents), _p(bl), _p(factors), _p(blocks), int(num_blocks), G, _p(group_of_hap), P, _p(focal_group),
             _p(cond_group), _p(ages) if ages is not None else None, E, _p(epochs), EF, _p(epochs_focal), _p(num), _p(denom)))
    return num, denom


def coalrate_accumulate(parents, branch_lengths, weights, blocks, num_blocks, group_vector_ids, group_vectors, num_groups,
                        epochs, sample_ages=None, device=True):
    """`CoalRate --mode local_ancestry` per-block sums (colate_coalrate_accumulate[_host]): parents / branch_lengths
    [T, 2N-1] (Relate labelling, root 2N-2), weights [T] (float64, bases), blocks [T], group_vector_ids [T] into
    group_vectors [S, N] (labels in [0, num_groups)); epochs float64 from 0, increasing; sample_ages [N] or None.
    Returns (num, denom), float64 [num_blocks, G, G, E], filled for g1 >= g2.  device=False: the host twin (bit for bit
    the same sums)."""
    parents = np.ascontiguousarray(parents, dtype=np.int32)
    group_vectors = np.ascontiguousarray(group_vectors, dtype=np.int32)
    if group_vectors.ndim != 2:
        raise ValueError("group_vectors must be [S, N]")
    S, N = group_vectors.shape
    T = parents.shape[0] if parents.ndim == 2 else 0
    if T and parents.shape[1] != 2 * N - 1:
        raise ValueError("parents must be [T, 2N-1]")
    bl = _f64(branch_lengths).reshape(T, 2 * N - 1) if T else np.zeros((0, 1))
    weights = _f64(weights).ravel()
    blocks = np.ascontiguousarray(blocks, dtype=np.int32).ravel()
    gv = np.ascontiguousarray(group_vector_ids, dtype=np.int32).ravel()
    if not (weights.size == blocks.size == gv.size == T):
        raise ValueError("weights, blocks and group_vector_ids must have one entry per tree")
    epochs = _f64(epochs).ravel()
    ages = None if sample_ages is None else _f64(sample_ages).ravel()
    if ages is not None and ages.size != N:
        raise ValueError("sample_ages must be [N]")
    E, G = epochs.size, int(num_groups)
    num = np.zeros((int(num_blocks), G, G, E))
    denom = np.zeros_like(num)
    fn = lib.colate_coalrate_accumulate if device else lib.colate_coalrate_accumulate_host
    check(fn(N, T, _p(parents), _p(bl), _p(weights), _p(blocks), int(num_blocks), _p(gv), S, _p(group_vectors), G,
             _p(ages) if ages is not None else None, E, _p(epochs), _p(num), _p(denom)))
    return num, denom


def coalrate_tree_accumulate(parents, branch_lengths, weights, blocks, num_blocks, epochs, sample_ages=None, device=True):
    """`CoalRate --mode tree` per-block sums (colate_coalrate_tree_accumulate[_host]): parents / branch_lengths [T, 2N-1]
    (Relate labelling, root 2N-2), weights [T] (float64, bases), blocks [T]; epochs float64 from 0, increasing; sample_ages
    [N] or None.  Returns (num, denom), float64 [num_blocks, E].  device=False: the host twin (bit for bit the same sums)."""
    parents = np.ascontiguousarray(parents, dtype=np.int32)
    if parents.ndim != 2 or parents.shape[1] % 2 != 1:
        raise ValueError("parents must be [T, 2N-1]")
    T, nn = parents.shape
    N = (nn + 1) // 2
    bl = _f64(branch_lengths).reshape(T, nn)
    weights = _f64(weights).ravel()
    blocks = np.ascontiguousarray(blocks, dtype=np.int32).ravel()
    if not (weights.size == blocks.size == T):
        raise ValueError("weights and blocks must have one entry per tree")
    epochs = _f64(epochs).ravel()
    ages = None if sample_ages is None else _f64(sample_ages).ravel()
    if ages is not None and ages.size != N:
        raise ValueError("sample_ages must be [N]")
    E = epochs.size
    num = np.zeros((int(num_blocks), E))
    denom = np.zeros_like(num)
    fn = lib.colate_coalrate_tree_accumulate if device else lib.colate_coalrate_tree_accumulate_host
    check(fn(N, T, _p(parents), _p(bl), _p(weights), _p(blocks), int(num_blocks), _p(ages) if ages is not None else None, E,
             _p(epochs), _p(num), _p(denom)))
    return num, denom


def _launch_shape(fn):
    out = np.zeros(5, dtype=np.int32)
    fn(_p(out))
    return dict(zip(("launches", "cpw_min", "cpw_max", "lanes_per_call", "lds"), (int(v) for v in out)))


def coalrate_launch_shape():
    """The first-kernel launches of this thread's last coalrate_accumulate(device=True) (diagnostic): their number, the
    smallest and largest calls per workgroup, the lanes per call, and whether the prefix counts lay in LDS (1 / 0).  All 0
    where nothing was launched."""
    return _launch_shape(lib.colate_coalrate_launch_shape)


def coalrate_tree_launch_shape():
    """The same for this thread's last coalrate_tree_accumulate(device=True); lds: whether the sort keys lay in LDS."""
    return _launch_shape(lib.colate_coalrate_tree_launch_shape)
