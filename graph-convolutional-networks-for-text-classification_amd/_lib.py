"""ctypes binding of libgcnk.so (the C-ABI declared in include/gcnk.h).

The shared library is built in-tree by ``__graft_entry__.build()`` (or
``make -C <package>/csrc``).  There is no fallback: if the library is missing
or fails to load, every op raises ``RuntimeError`` — the hot path never
silently runs anywhere but the HIP kernels.
"""
import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
PRODUCT_LIB = os.path.join(_HERE, "libgcnk.so")
VARIANT_DIR = os.path.join(os.path.dirname(_HERE), "_variants")


def _resolve_lib():
    """The in-tree library, unless GCNK_LIB names an experiment variant built by
    `make -C <pkg>/csrc variant` (it must live in <repo>/_variants/; anything
    else is refused, so a stale export cannot swap in a foreign binary).  A
    variant is announced on stderr; tests/conftest.py refuses to run on one."""
    want = os.environ.get("GCNK_LIB")
    if not want:
        return PRODUCT_LIB
    path = os.path.realpath(want)
    if os.path.dirname(path) != os.path.realpath(VARIANT_DIR):
        raise RuntimeError(f"GCNK_LIB={want}: only experiment variants in {VARIANT_DIR} may replace {PRODUCT_LIB}")
    import sys
    print(f"[gcnk] loading experiment variant {path} (not the product library)", file=sys.stderr)
    return path


LIB_PATH = _resolve_lib()
ABI_VERSION = 13

# C-ABI return codes (gcnk.h)
OK, EARG, EUNSUP, EHIP = 0, -1, -2, -3

# SpMM epilogues (gcnk.h GCNK_EPI_*)
EPI_NONE, EPI_BIAS, EPI_BIAS_RELU, EPI_BIAS_RELU_DROP, EPI_BIAS_RELU_HASH = 0, 1, 2, 3, 4
# GEMM epilogues (gcnk.h GCNK_GEMM_EPI_*)
GEMM_EPI_NONE, GEMM_EPI_BIAS, GEMM_EPI_BIAS_RELU, GEMM_EPI_MASK_POS = 0, 1, 2, 5
# gcnk_gemm_route's families and flags (gcnk.h GCNK_GEMM_ROUTE_*)
(GEMM_ROUTE_NARROW, GEMM_ROUTE_SKINNY, GEMM_ROUTE_SHORTK, GEMM_ROUTE_SMALLM, GEMM_ROUTE_TILED_N16,
 GEMM_ROUTE_TILED) = 1, 2, 3, 4, 5, 6
GEMM_ROUTE_SPLIT, GEMM_ROUTE_PTR_FETCH = 1, 2
# gcnk_spmm_route's aligned16 mask (gcnk.h GCNK_SPMM_ALIGNED_*)
SPMM_ALIGNED_B, SPMM_ALIGNED_C, SPMM_ALIGNED_BIAS, SPMM_ALIGNED_WORKSPACE, SPMM_ALIGNED_ALL = 1, 2, 4, 8, 15

_vp, _i32, _i64, _u64, _f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float
_f64 = ctypes.c_double
# gcnk_adam_f32 (gcnk.h GCNK_ADAM_*)
ADAM_MAX_TENSORS, ADAM_CHUNK, ADAM_ZERO_GRAD, ADAM_HOLD_STEP = 8, 2048, 1, 2


class AdamTensor(ctypes.Structure):
    """gcnk.h gcnk_adam_tensor"""
    _fields_ = [("p", _vp), ("g", _vp), ("m", _vp), ("v", _vp), ("numel", _i64)]


class EpochState(ctypes.Structure):
    """gcnk.h gcnk_epoch_state (32 bytes on the device)"""
    _fields_ = [("epoch", _i32), ("stopped", _i32), ("stop_epoch", _i32), ("counter", _i32), ("best", _f64),
                ("arrivals", _i32), ("reserved", _i32)]


# gcnk_epoch_tail_f32's stop reasons (gcnk.h GCNK_EPOCH_STOP_*)
EPOCH_STOP_PATIENCE, EPOCH_STOP_MAX_EPOCH = 1, 2
# gcnk_keep_best_f32 (gcnk.h GCNK_KEEP_*)
KEEP_MAX_TENSORS, KEEP_CHUNK, KEEP_HOLD_STATE = 8, 8192, 1


class KeepTensor(ctypes.Structure):
    """gcnk.h gcnk_keep_tensor"""
    _fields_ = [("src", _vp), ("dst", _vp), ("numel", _i64)]


class KeepState(ctypes.Structure):
    """gcnk.h gcnk_keep_state (16 bytes on the device)"""
    _fields_ = [("seen", _i32), ("best", _i32), ("arrivals", _i32), ("copies", _i32)]


class LaunchTables:
    """The host tensor tables of a multi-tensor entry point (gcnk_adam_f32,
    gcnk_keep_best_f32): rows of the ctypes ``struct`` (a tensor's pointers,
    then ``numel``), at most ``per_call`` of them a launch."""

    def __init__(self, struct, per_call):
        self.struct, self.per_call, self._cache = struct, per_call, {}   # launch -> (pointers, struct array)
        self.clear = self._cache.clear

    def launches(self, ptrs, numels, first=0, last=True):
        """[(table, rows, hold)] for the tensors with pointer tuples ``ptrs``, the
        launches numbered from ``first``; a table is rebuilt only when one of
        its pointers changed.  ``hold`` (the entry point's HOLD flag is due): on
        every launch but the last, and on that too unless ``last``."""
        out = []
        for i in range(0, len(ptrs), self.per_call):
            key, li = tuple(ptrs[i:i + self.per_call]), first + len(out)
            if self._cache.get(li, (None,))[0] != key:
                self._cache[li] = (key, (self.struct * len(key))(*[(*p, n) for p, n in zip(key, numels[i:])]))
            out.append((self._cache[li][1], len(key), not last or i + self.per_call < len(ptrs)))
        return out


def epoch_row_words(nclass):
    """gcnk.h GCNK_EPOCH_ROW_WORDS: train_loss | val_loss | TP | FP | FN | correct"""
    return 3 * nclass + 3


# the nine epilogue arguments of the entry points that end in the SpMM's fused epilogue:
# bias, epilogue, drop_mask, ldm, drop_scale, keep_prob, seed, offset, rng_base
_EPI_ARGS = [_vp, _i32, _vp, _i64, _f32, _f32, _u64, _u64, _vp]

# name -> (restype, argtypes); every symbol include/gcnk.h declares
SIGNATURES = {
    "gcnk_abi_version": (ctypes.c_int, []),
    "gcnk_debug_set_stamps": (ctypes.c_int, [_vp]),
    "gcnk_last_error": (ctypes.c_char_p, []),
    "gcnk_spmm_groups": (_i32, [_i32, _i32]),
    "gcnk_spmm_default_ipc": (_i32, [_i32, _i64, _i32, _i32]),
    # rowptr, colind, M, K, nnz, ipc, groups, dense_threshold, stream
    "gcnk_spmm_plan_bytes": (_i64, [_vp, _vp, _i32, _i32, _i64, _i32, _i32, _f32, _vp]),
    # rowptr, colind, val, M, K, nnz, ipc, groups, dense_threshold, plan, plan_bytes, stream
    "gcnk_spmm_plan_build": (ctypes.c_int, [_vp, _vp, _vp, _i32, _i32, _i64, _i32, _i32, _f32, _vp, _i64, _vp]),
    "gcnk_spmm_plan_bytes_host": (_i64, [_vp, _vp, _i32, _i32, _i64, _i32, _i32, _f32]),
    "gcnk_spmm_plan_build_host": (ctypes.c_int, [_vp, _vp, _vp, _i32, _i32, _i64, _i32, _i32, _f32, _vp, _i64]),
    "gcnk_spmm_plan_query": (ctypes.c_int, [_vp, _vp, _vp]),
    "gcnk_spmm_workspace_bytes": (_i64, [_vp, _i32]),
    "gcnk_spmm_counter_bytes": (_i64, [_vp]),
    "gcnk_spmm_csr_f32": (ctypes.c_int, [
        _vp, _vp,                 # plan (device), plan header (host, 16 words)
        _vp, _i64, _i32,          # B, ldb, F
        _vp, _i64,                # C, ldc
        *_EPI_ARGS,
        _vp, _i64,                # workspace, workspace_bytes
        _vp, _i64,                # counters, counter_bytes
        _i32, _vp,                # lanes_hint, stream
    ]),
    "gcnk_spmm_csr_f32_part": (ctypes.c_int, [
        _vp, _vp,                 # plan (device), plan header (host, 16 words)
        _vp, _i64, _i32,          # B, ldb, F
        _vp, _i64,                # C, ldc
        *_EPI_ARGS,
        _vp, _i64,                # workspace, workspace_bytes
        _vp, _i64,                # counters, counter_bytes
        _i32, _i32, _vp,          # lanes_hint, part, stream
    ]),
    "gcnk_spmm_proj_f32": (ctypes.c_int, [
        _vp, _vp,                 # plan, plan header
        _vp, _i64, _i32,          # B, ldb, F
        _vp, _i64,                # C (nullable), ldc
        *_EPI_ARGS,
        _vp, _i64, _i32, _vp, _i64,  # W, ldw, P, C2, ldc2
        _vp, _i64,                # workspace, workspace_bytes
        _vp, _i64,                # counters, counter_bytes
        _i32, _vp,                # lanes_hint, stream
    ]),
    # plan header (host), F, ldb, ldc, aligned16 mask, lanes_hint, P, part, out16
    "gcnk_spmm_route": (ctypes.c_int, [_vp, _i32, _i64, _i64, _i32, _i32, _i32, _i32, _vp]),
    "gcnk_gemm_workspace_bytes": (_i64, [_i32, _i32, _i32, _i32]),
    "gcnk_gemm_f32": (ctypes.c_int, [
        _i32, _i32, _i32, _i32, _i32,   # transA, transB, M, N, K
        _vp, _i64, _vp, _i64,           # A, lda, B, ldb
        _vp, _i64,                      # C, ldc
        _vp, _i32, _vp, _i64, _f32,     # bias, epilogue, R, ldr, scale
        _i32, _vp, _i64, _vp,           # split_k, workspace, workspace_bytes, stream
    ]),
    # transA, transB, M, N, K, lda, ldb, a_aligned16, b_aligned16, split_k, out4
    "gcnk_gemm_route": (ctypes.c_int, [_i32, _i32, _i32, _i32, _i32, _i64, _i64, _i32, _i32, _i32, _vp]),
    "gcnk_colsum_workspace_bytes": (_i64, [_i32, _i32]),
    "gcnk_colsum_f32": (ctypes.c_int, [_vp, _i64, _i32, _i32, _vp, _vp, _i64, _vp]),
    "gcnk_gcn_bwd2_workspace_bytes": (_i64, [_i32, _i32, _i32]),
    "gcnk_gcn_bwd2_f32": (ctypes.c_int, [
        _vp, _i64, _vp, _i64, _vp, _i64,   # H, ldh, gS, ldgs, W, ldw
        _vp, _i64, _i32, _i32, _i32, _f32,  # G, ldg, M, N, P, scale
        _vp, _i64, _vp, _vp, _vp,          # gZ1, ldz, gW, gb1, gb2
        _vp, _i64, _vp]),                  # workspace, bytes, stream
    # M, N, P, ldh, ldz, h_align, z_align, ldgs, has_g, ldg, ldw, w_aligned16, out9
    "gcnk_gcn_bwd2_route": (ctypes.c_int, [_i32, _i32, _i32, _i64, _i64, _i32, _i32, _i64, _i32, _i64, _i64, _i32, _vp]),
    "gcnk_stream_copy_f32": (ctypes.c_int, [_vp, _vp, _i64, _vp]),
    "gcnk_debug_poison_lds": (ctypes.c_int, [ctypes.c_uint32, _vp]),
    "gcnk_hubfactor_lds_bytes": (_i64, [_i32, _i32, _i32, _i32, _i32]),
    "gcnk_hubfactor_gc1_f32": (ctypes.c_int, [
        _i32, _i32, _i32, _i32, _i32,     # M, F, Kc, nhub, P
        _vp, _i64, _vp, _i64, _i32,       # U, ldu, W, ldw, k0
        _vp, _i64, _vp, _i32,             # S, lds, rec, rec_words
        *_EPI_ARGS,
        _vp, _i64, _vp, _i64, _vp, _i64,  # W2, ldw2, H, ldh, C2, ldc2
        _vp]),                            # stream
    # F, Kc, nhub, rec_words, P, ldu, u_aligned16, out6
    "gcnk_hubfactor_gc1_route": (ctypes.c_int, [_i32, _i32, _i32, _i32, _i32, _i64, _i32, _vp]),
    "gcnk_hubfactor_gc2_f32": (ctypes.c_int, [
        _i32, _i32, _i32, _vp, _i32,      # M, H, P, rec, rec_words
        _vp, _vp, _vp, _vp, _vp, _vp,     # diag, pre, hub_ids (host), hub_rp (host), hub_ci, hub_val
        _vp, _i64, _vp, _vp, _i64,        # S2, lds2, b2, out, ldo
        _vp]),                            # stream
    "gcnk_score_docs_f32": (ctypes.c_int, [
        _i32, _i32, _i32, _i32, _i32, _i32,   # B, F, Kc, H, P, k0
        _vp, _i64, _vp, _i64,             # x, ldx, a, lda
        _vp, _i64, _vp, _i64,             # W1, ldw1, S_T, lds
        _vp, _i64, _vp, _i64,             # W2, ldw2, S2_T, lds2
        _vp, _vp, _vp,                    # dh (float64), b1, b2
        _vp, _i64, _vp, _vp]),            # out, ldo, labels (int32), stream
    # F, Kc, H, P, out8
    "gcnk_score_docs_route": (ctypes.c_int, [_i32, _i32, _i32, _i32, _vp]),
    # rowptr, colind, val, M, hub_index, perm, diag, pre, stream
    "gcnk_factor_diag_f32": (ctypes.c_int, [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "gcnk_dense_gc1_f32": (ctypes.c_int, [
        _i32, _i32, _i32, _i32,           # M, K, F, P
        _vp, _i64, _vp, _i64,             # AX, ldax, W1, ldw1
        *_EPI_ARGS,
        _vp, _i64, _vp, _i64, _vp, _i64,  # W2, ldw2, H, ldh, C2, ldc2
        _vp]),                            # stream
    "gcnk_aggregate_f32": (ctypes.c_int, [_vp, _vp, _vp, _i32, _vp, _i64, _i32, _vp, _i64, _i32, _vp]),
    # record (host struct gcnk_gcn_fwd), W1, b1, W2, b2, out, ldo, H1, ldh, epilogue, mask, ldm, scale,
    # keep_prob, seed, offset, rng_base, stream
    "gcnk_gcn_forward_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _i32, _vp, _i64, _f32,
                                            _f32, _u64, _u64, _vp, _vp]),
    "gcnk_gcn_fwd_layout": (_i32, [_vp, _i32]),
    "gcnk_factor_u_f32": (ctypes.c_int, [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _i64, _i32, _vp, _i64, _i32, _vp]),
    "gcnk_factor_records": (ctypes.c_int, [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp]),
    "gcnk_factor_analyze_workspace_bytes": (_i64, [_i32, _i32]),
    # rowptr, colind, M, hmin, x_rowptr, x_colind, x_val, x_dense, ldx, K, max_hubs, info, hubs, cnt (host),
    # workspace, bytes, stream
    "gcnk_factor_analyze": (ctypes.c_int, [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp,
                                           _vp, _i64, _vp]),
    "gcnk_factor_xl_f32": (ctypes.c_int, [_vp, _vp, _vp, _i32, _vp, _i32, _i32, _vp, _i64, _i32, _vp]),
    "gcnk_csr_gather_rows": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "gcnk_dense_gather_rows_f32": (ctypes.c_int, [_vp, _i64, _i32, _vp, _i32, _vp, _i64, _vp]),
    "gcnk_gcn_backward_f32": (ctypes.c_int, [_vp, _vp, _vp, _i64, _vp, _f32, _vp, _vp, _vp, _vp, _vp]),
    "gcnk_class_stats": (ctypes.c_int, [_vp, _i64, _vp, _vp, _i64, _i32, _vp, _vp]),
    # idx, n, M, counts, stream
    "gcnk_ce_row_counts": (ctypes.c_int, [_vp, _i64, _i32, _vp, _vp]),
    "gcnk_ce_workspace_bytes": (_i64, [_i32, _i32]),
    # logits, ld, M, P, target, counts, n, loss, lse, workspace, workspace_bytes, stream
    "gcnk_ce_forward_f32": (ctypes.c_int, [_vp, _i64, _i32, _i32, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp]),
    # logits, ld, M, P, target, counts, n, lse, grad_out, dlogits, ldd, stream
    "gcnk_ce_backward_f32": (ctypes.c_int, [_vp, _i64, _i32, _i32, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp]),
    # tensor table (host, AdamTensor[ntensors]), ntensors, lr, beta1, beta2, eps, weight_decay, state, flags, stream
    "gcnk_adam_f32": (ctypes.c_int, [_vp, _i32, _f64, _f64, _f64, _f64, _f64, _vp, _i32, _vp]),
    # gcnk_adam_f32's arguments, then gate before stream
    "gcnk_adam_gated_f32": (ctypes.c_int, [_vp, _i32, _f64, _f64, _f64, _f64, _f64, _vp, _i32, _vp, _vp]),
    "gcnk_epoch_tail_workspace_bytes": (_i64, [_i32, _i32]),
    # logits, ld, M, P, target, counts, n, train_loss, state, history, max_epoch, patience, delta, workspace,
    # workspace_bytes, stream
    "gcnk_epoch_tail_f32": (ctypes.c_int, [_vp, _i64, _i32, _i32, _vp, _vp, _i64, _vp, _vp, _vp, _i32, _i32, _f64,
                                           _vp, _i64, _vp]),
    # tensor table (host, KeepTensor[ntensors]), ntensors, epoch_state, state, flags, stream
    "gcnk_keep_best_f32": (ctypes.c_int, [_vp, _i32, _vp, _vp, _i32, _vp]),
    "gcnk_edgelist_size": (ctypes.c_int, [ctypes.c_char_p, _vp, _vp]),
    "gcnk_edgelist_csr": (ctypes.c_int, [ctypes.c_char_p, _i64, _i64, _vp, _vp, _vp]),
    "gcnk_csr_to_dense": (ctypes.c_int, [_vp, _vp, _vp, _i32, _i32, _vp, _i64, _vp]),
    "gcnk_bernoulli_mt19937": (ctypes.c_int, [_vp, _vp, _vp, _i64, ctypes.c_double, _vp, _i32]),
    "gcnk_bernoulli_mt19937_start": (ctypes.c_int, [_vp, _vp, _vp, _i64, ctypes.c_double, _vp, _vp]),
    "gcnk_bernoulli_mt19937_wait": (ctypes.c_int, [_vp]),
    "gcnk_sym_normalize_workspace_bytes": (_i64, [_i32, _i64]),
    "gcnk_sym_normalize": (ctypes.c_int, [_vp, _vp, _vp, _i32, _i64, _vp, _vp, _vp, _vp, _i64, _vp]),
    "gcnk_topic_graph_chunk": (_i32, []),
    "gcnk_topic_graph_max_topics": (_i32, []),
    "gcnk_topic_graph_nnz_bound": (_i64, [_i32, _i32, _i32]),       # D, K, has_sim
    "gcnk_topic_graph_workspace_bytes": (_i64, [_i32, _i32]),       # D, K
    "gcnk_topic_graph_build": (ctypes.c_int, [
        _vp, _i32, _i64, _vp, _i32, _i64,   # theta, theta_f32, ldt, sim (nullable), sim_f32, lds
        _i32, _i32, _f64, _f64,             # D, K, doc_topic_threshold, topic_topic_threshold
        _vp, _vp, _vp, _i64, _vp,           # rowptr, colind, val, capacity, edges (nullable, int32[2])
        _vp, _i64, _vp]),                   # workspace, workspace_bytes, stream
    # emb, emb_f32, lde, K, dim, sim (float64), lds, stream
    "gcnk_topic_cosine_f64": (ctypes.c_int, [_vp, _i32, _i64, _i32, _i32, _vp, _i64, _vp]),
    "gcnk_lda_max_topics": (_i32, []),
    "gcnk_lda_tile_words": (_i32, []),
    "gcnk_lda_docs_per_block": (_i32, []),
    # components / exp_topic_word (float64 [K x V]), its row stride, K, V, table, ldt, stream
    "gcnk_lda_exp_dirichlet_f64": (ctypes.c_int, [_vp, _i64, _i32, _i32, _vp, _i64, _vp]),
    "gcnk_lda_table_from_exp_f64": (ctypes.c_int, [_vp, _i64, _i32, _i32, _vp, _i64, _vp]),
    "gcnk_lda_estep_f64": (ctypes.c_int, [
        _vp, _vp, _vp, _i32,                # indptr, indices, counts, counts_kind (0 f64, 1 i32, 2 i64)
        _i32, _i32, _i32, _vp, _i64,        # B, V, K, table, ldt
        _f64, _f64, _i32,                   # alpha, tol, max_iter
        _vp, _i64, _vp, _vp,                # theta, ldth, gamma, iters (int32[B]); each nullable
        _vp, _i64, _vp, _i64, _f64,         # x, ldx, a, lda (nullable together), threshold
        _vp]),                              # stream
    "gcnk_lda_words_per_block": (_i32, []),
    "gcnk_lda_estep_fit_f64": (ctypes.c_int, [
        _vp, _vp, _vp, _i32,                # indptr, indices, counts, counts_kind
        _i32, _i32, _i32, _vp, _i64,        # B, V, K, table, ldt
        _f64, _f64, _i32,                   # alpha, tol, max_iter
        _vp, _i64, _i64, _vp,               # gamma0, ldg0, nnz, ratio (float64[nnz])
        _vp, _i64, _vp, _i64, _vp,          # etheta, lde, gamma, ldg, iters (the last two pointers nullable)
        _vp]),                              # stream
    "gcnk_lda_mstep_f64": (ctypes.c_int, [
        _vp, _vp, _vp, _i64,                # wptr, pos, doc, nnz
        _vp, _vp, _i64,                     # ratio, etheta, lde
        _i32, _i32, _i32, _vp, _i64,        # B, V, K, table, ldt
        _f64, _vp, _i64, _vp]),             # eta, lambda, ldl, stream
    "gcnk_lda_mstep_online_f64": (ctypes.c_int, [
        _vp, _vp, _vp, _i64, _i32, _i32,    # wptr, pos, doc, nnz, doc_lo, doc_hi
        _vp, _vp, _i64,                     # ratio, etheta, lde
        _i32, _i32, _i32, _vp, _i64,        # B, V, K, table, ldt
        _f64, _f64, _f64,                   # eta, rho, doc_ratio
        _vp, _i64, _vp]),                   # lambda (in place), ldl, stream
    "gcnk_csr_transpose_workspace_bytes": (_i64, [_i32, _i32, _i64]),
    "gcnk_coo_to_csr_workspace_bytes": (_i64, [_i64, _i32, _i32]),
    "gcnk_coo_to_csr": (ctypes.c_int, [_vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _i64, _vp]),
    "gcnk_csr_transpose": (ctypes.c_int, [_vp, _vp, _vp, _i32, _i32, _i64, _vp, _vp, _vp, _vp, _i64, _vp]),
}

# added within ABI 13 (gc2 from the hub factor, the backward's and the factored gc1's route reports): absent from
# variants of an older tree
NEWER_THAN_SOME_VARIANTS = ("gcnk_hubfactor_gc2_f32", "gcnk_factor_diag_f32", "gcnk_gcn_bwd2_route",
                            "gcnk_hubfactor_gc1_route", "gcnk_score_docs_f32", "gcnk_score_docs_route",
                            "gcnk_spmm_route", "gcnk_topic_graph_chunk", "gcnk_topic_graph_max_topics",
                            "gcnk_topic_graph_nnz_bound", "gcnk_topic_graph_workspace_bytes",
                            "gcnk_topic_graph_build", "gcnk_topic_cosine_f64", "gcnk_lda_max_topics",
                            "gcnk_lda_tile_words", "gcnk_lda_docs_per_block", "gcnk_lda_exp_dirichlet_f64",
                            "gcnk_lda_table_from_exp_f64", "gcnk_lda_estep_f64", "gcnk_lda_words_per_block",
                            "gcnk_lda_estep_fit_f64", "gcnk_lda_mstep_f64", "gcnk_lda_mstep_online_f64")

_lock = threading.Lock()
_lib = None


class GcnkError(RuntimeError):
    """Raised when a libgcnk entry point returns a non-zero code."""


def load():
    """Load libgcnk.so once and bind every declared symbol; raise if absent."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"libgcnk.so not found at {LIB_PATH}: build it with __graft_entry__.build() "
                "or `make -C <package>/csrc` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name, None)
            if fn is None:
                # an experiment variant built from an older csrc (an A/B's parent library)
                # may lack the newest entry points: their callers test for them
                if LIB_PATH == PRODUCT_LIB or name not in NEWER_THAN_SOME_VARIANTS:
                    raise RuntimeError(f"{LIB_PATH} does not export {name}")
                continue
            fn.restype = res
            fn.argtypes = args
        v = lib.gcnk_abi_version()
        if v != ABI_VERSION:
            raise RuntimeError(f"libgcnk ABI version {v} != expected {ABI_VERSION}")
        _lib = lib
        return lib


def stream(device):
    """The current stream of ``device`` as the ``void* stream`` every launch takes."""
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def check(rc, what):
    if rc != OK:
        msg = load().gcnk_last_error().decode(errors="replace")
        kind = {EARG: "bad argument", EUNSUP: "unsupported", EHIP: "HIP error"}.get(rc, "error")
        raise GcnkError(f"{what} failed ({kind}, rc={rc}): {msg} [{LIB_PATH}]")
