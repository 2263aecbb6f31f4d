"""ctypes binding of include/cyclevae_hip.h (libcyclevae_hip.so).

Pointer-level and framework-agnostic: every buffer argument is an integer device address
(`tensor.data_ptr()`); streams are integer hipStream_t handles.  There is no fallback: if the shared
library is missing or its ABI version differs, loading raises.
"""
import ctypes as C
import os

ABI_VERSION = 10
FLAG_PERSISTENT = 1
FLAG_PROFILE = 2
FLAG_GENERIC_STEP = 4
FLAG_STEP_TIMING = 8
FLAG_HOISTED_FRONTEND = 32
FLAG_SPLIT_F16 = 256
FLAG_EXACT3 = 512
STATUS_RANGE = 7        # CVAE_STATUS_RANGE: an operand of a limb-operand eval kernel was outside the window of its fp16 limbs (ABI 8)
STATUS_RANGE_WORD = 3   # the status word that carries it (word 0: time-outs, status 5)
CLAMP_LAPLACE = 1 << 30     # OR into a clamp_lat_dim argument: clamp_vae_laplace's floor (gru_vae.py:417) instead of ln(1e-6)
DRAW_LAPLACE = 1 << 30      # OR into a lat_dim argument (pass_input, cycle_forward*, latent_mean, sample_cat*, stage4_loss, trainlog_window's L): the Laplace
                            # posterior -- z = mu + exp(s) * u(eps), loss_vae_laplace's KL (gru_vae.py:101-112, :130-139)
POSTERIORS = ("gauss", "laplace")


def posterior_flags(posterior, lat_dim):
    """(lat_dim argument of the draws and the loss, clamp_lat_dim argument of the encoder passes) of a posterior choice."""
    if posterior not in POSTERIORS:
        raise ValueError("posterior=%r: expected one of %s" % (posterior, ", ".join(repr(p) for p in POSTERIORS)))
    if posterior == "laplace":
        return lat_dim | DRAW_LAPLACE, lat_dim | CLAMP_LAPLACE
    return lat_dim, lat_dim

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.environ.get("CYCLEVAE_LIB") or os.path.join(_HERE, "libcyclevae_hip.so")   # (variable: A/B builds of the same library)

_fp = C.c_void_p


class NetDesc(C.Structure):
    _fields_ = [("in_dim", C.c_int32), ("out_dim", C.c_int32), ("hidden", C.c_int32), ("kernel_size", C.c_int32),
                ("layers", C.c_int32), ("has_scale_in", C.c_int32), ("has_scale_out", C.c_int32)]


WEIGHT_FIELDS = ("scale_in_w", "scale_in_b", "conv0_w", "conv0_b", "conv1_w", "conv1_b", "w_ih", "w_hh", "b_ih",
                 "b_hh", "out_w", "out_b", "scale_out_w", "scale_out_b", "conv2_w", "conv2_b")      # conv2_*: ABI 10, dilation_size == 3

# C field -> reference state_dict key
STATE_KEYS = {"scale_in_w": "scale_in.weight", "scale_in_b": "scale_in.bias", "conv0_w": "conv.conv.0.weight",
              "conv0_b": "conv.conv.0.bias", "conv1_w": "conv.conv.1.weight", "conv1_b": "conv.conv.1.bias",
              "conv2_w": "conv.conv.2.weight", "conv2_b": "conv.conv.2.bias",
              "w_ih": "gru.weight_ih_l0", "w_hh": "gru.weight_hh_l0", "b_ih": "gru.bias_ih_l0",
              "b_hh": "gru.bias_hh_l0", "out_w": "out_1.weight", "out_b": "out_1.bias",
              "scale_out_w": "scale_out.weight", "scale_out_b": "scale_out.bias"}


class NetWeights(C.Structure):
    _fields_ = [(f, _fp) for f in WEIGHT_FIELDS]


GRAD_FIELDS = ("conv0_w", "conv0_b", "conv1_w", "conv1_b", "w_ih", "w_hh", "b_ih", "b_hh", "out_w", "out_b")


class GruLayer(C.Structure):
    """The four tensors of one GRU layer l >= 1 (cvae_gru_layer, ABI 7)."""
    _fields_ = [(f, _fp) for f in ("w_ih", "w_hh", "b_ih", "b_hh")]


def upper_layer_keys(n_layers):
    """state_dict keys of the GRU layers 1 .. n_layers-1, per layer in the field order of GruLayer."""
    return [tuple("gru.%s_l%d" % (k, l) for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")) for l in range(1, n_layers)]


DEEP_PER_STEP, DEEP_GENERIC, DEEP_RESIDENT = 0, 1, 2      # cvae_plan_pass_deep
EVAL_PER_STEP, EVAL_GENERIC, EVAL_V2, EVAL_V4, EVAL_V5, EVAL_V6, EVAL_LL, EVAL_V6H = range(8)      # cvae_plan_pass (cvae_eval_form)
# cvae_plan_train_pass: the forward / reverse forms (FwdForm / BwdForm of csrc/cvae_train.inc) and the fields of its answer
TRAIN_FWD_LL, TRAIN_FWD_W3, TRAIN_FWD_X3, TRAIN_FWD_X3H, TRAIN_FWD_PAIR, TRAIN_FWD_FP32, TRAIN_FWD_STEPS = range(7)
TRAIN_BWD_LL, TRAIN_BWD_W3, TRAIN_BWD_X3, TRAIN_BWD_PAIR, TRAIN_BWD_STEPS = range(5)
TRAIN_PLAN_FIELDS = ("Bp", "fwd", "fwd_rts", "fwd_tiles", "fwd_col_tiles", "fwd_full_writes", "bwd", "bwd_rts", "bwd_per_launch", "bwd_tiles",
                     "bwd_writes_gates", "variants")
MAX_LAYERS = 8                                              # CVAE_DEEP_MAX_LAYERS


class NetGrads(C.Structure):
    _fields_ = [(f, _fp) for f in GRAD_FIELDS]


class Seg(C.Structure):
    _fields_ = [("ptr", _fp), ("width", C.c_int32), ("row_stride", C.c_int32)]


class PassInput(C.Structure):
    _fields_ = [("seg0", Seg), ("seg1", Seg), ("lat", _fp), ("lat_dim", C.c_int32), ("eps", _fp),
                ("seed", C.c_uint64), ("draw_id", C.c_uint64), ("frames", C.c_int32), ("n_draws", C.c_int32),
                ("ctx_before", C.c_int32), ("ctx_after", C.c_int32), ("draw_frame0", C.c_int64), ("eps_draw_stride", C.c_int64)]


class DtwProblem(C.Structure):
    """cvae_dtw_problem: one alignment of cvae_dtw_batch (device addresses; aligned may be None)."""
    _fields_ = [("org", _fp), ("trg", _fp), ("ld_org", C.c_int64), ("ld_trg", C.c_int64), ("T1", C.c_int32), ("T2", C.c_int32),
                ("D", C.c_int32), ("mcd", C.c_int32), ("aligned", _fp), ("twf", _fp), ("frames", _fp), ("mean_out", _fp)]


STAT_GV, STAT_MCD_SPC, STAT_MCD_L1, STAT_KL, STAT_GATHER64, STAT_LATDIST = range(6)      # cvae_stat_job.kind
STAT_MEANSTD64, STAT_MCD64 = 6, 7       # stage 5: (np.mean, np.std) of an f64 vector / of the frame-wise mel-cd of two f64 matrices
STAT_KL_LAPLACE = 8                     # STAT_KL's operands, loss_vae_laplace's KL (the Laplace posterior's loss_lat_* figures)


class StatJob(C.Structure):
    """cvae_stat_job: one reduction of cvae_eval_stats."""
    _fields_ = [("kind", C.c_int32), ("rows", C.c_int32), ("c0", C.c_int32), ("c1", C.c_int32), ("src_rows", C.c_int32),
                ("pad_", C.c_int32), ("a", _fp), ("b", _fp), ("lda", C.c_int64), ("ldb", C.c_int64), ("idx", _fp), ("dst", _fp),
                ("out_off", C.c_int64)]


class LatMeanJob(C.Structure):
    """cvae_latmean_job: one latent mean of cvae_latent_mean (device addresses; eps may be None)."""
    _fields_ = [("lat", _fp), ("eps", _fp), ("draw_id", C.c_uint64), ("frames", C.c_int32), ("pad_", C.c_int32), ("out", _fp)]


class Mc2eJob(C.Structure):
    """cvae_mc2e_job: one matrix of cvae_mc2e_batch (device addresses)."""
    _fields_ = [("mc", _fp), ("is_f64", C.c_int32), ("T", C.c_int32), ("D", C.c_int32), ("pad_", C.c_int32), ("ld", C.c_int64), ("e_out", _fp)]


class GemmCase(C.Structure):
    """cvae_gemm_case: one training GEMM / column sum for cvae_selftest_gemm (device addresses; include/cyclevae_hip.h)."""
    _fields_ = [("kind", C.c_int32), ("accumulate", C.c_int32), ("use_split", C.c_int32), ("M", C.c_int32), ("N", C.c_int32),
                ("K", C.c_int32), ("seglen", C.c_int32), ("mask_B", C.c_int32), ("mask_Bp", C.c_int32), ("mask_T", C.c_int32),
                ("lda", C.c_int64), ("ldb", C.c_int64), ("ldc", C.c_int64), ("segstride", C.c_int64),
                ("a_lo", C.c_int64), ("a_hi", C.c_int64), ("b_lo", C.c_int64), ("b_hi", C.c_int64), ("c_hi", C.c_int64),
                ("A", _fp), ("B", _fp), ("bias", _fp), ("mask", _fp), ("C", _fp)]


GEMM_NT, GEMM_TN, GEMM_KS, GEMM_COLSUM = 0, 1, 2, 3      # cvae_gemm_case.kind
SELFTEST_GEMM_CNT = 4096                                 # arrival counters at the end of cvae_selftest_gemm's work space

DEC_MODPOW, DEC_GATHER = 0, 1       # cvae_decode_job.kind


class DecodeJob(C.Structure):
    """cvae_decode_job: one mod_pow / GV post-filter / difference, or one f64 gather, of cvae_decode_jobs (device addresses)."""
    _fields_ = [("kind", C.c_int32), ("T", C.c_int32), ("D", C.c_int32), ("c_f64", C.c_int32), ("ref_f64", C.c_int32),
                ("src_rows", C.c_int32), ("c0", C.c_int32), ("c1", C.c_int32), ("c", _fp), ("ldc", C.c_int64), ("e_ref", _fp), ("e_c", _fp),
                ("gv", _fp), ("cvgv", _fp), ("x", _fp), ("g", _fp), ("var", _fp), ("dpow", _fp), ("ref", _fp), ("ldref", C.c_int64),
                ("diff", _fp), ("idx", _fp)]


TRAINLOG_MAX_CYC, TRAINLOG_MAX_UTT = 8, 128       # CVAE_TRAINLOG_MAX_CYC, CVAE_TRAINLOG_MAX_UTT
TRAINLOG_SLOTS = ("lat", "rec", "cv", "latcv", "reccyc")      # cvae_trainlog_window_args.traj[i][k] (stage4.PASS_SLOTS)
TRAINLOG_REC = 9                                    # doubles per (cycle, utterance) record


class MoveJob(C.Structure):
    """cvae_move_job: one strided row copy of cvae_stream_move (device addresses, strides in floats)."""
    _fields_ = [("dst", _fp), ("src", _fp), ("rows", C.c_int32), ("width", C.c_int32), ("dst_stride", C.c_int64), ("src_stride", C.c_int64)]


class TrainlogWindowArgs(C.Structure):
    """cvae_trainlog_window_args (device addresses; flen_acc, s_idx, e_idx, selected: HOST arrays the call reads before it returns)."""
    _fields_ = [("traj", (_fp * 5) * TRAINLOG_MAX_CYC), ("x_win", _fp), ("x_row_stride", C.c_int64), ("x_utt_stride", C.c_int64),
                ("spcidx", _fp), ("spc_ld", C.c_int64), ("flen_acc", _fp), ("s_idx", _fp), ("e_idx", _fp), ("selected", _fp),
                ("n_cyc", C.c_int32), ("B", C.c_int32), ("T", C.c_int32), ("D", C.c_int32), ("L", C.c_int32), ("stdim", C.c_int32),
                ("src_idx_s", C.c_int32), ("acc_rows", C.c_int32), ("acc", _fp * 4), ("rec_out", _fp)]


class CvaeError(RuntimeError):
    pass


class CvaeRangeError(CvaeError):
    """STATUS_RANGE: the passes since the last check ran the limb-operand kernels on a value their fp16 limbs cannot carry."""


class CycleState(C.Structure):
    _fields_ = [("y_enc", _fp), ("y_dec", _fp), ("h_enc", _fp), ("h_dec", _fp)]


class _Bound(object):
    """The shared library's entry points with THIS object's context as their first argument (ABI 6: every entry point but
    cvae_last_error_string / cvae_abi_version / cvae_ctx_create takes the handle).  `lib.lib.cvae_xyz(args...)` therefore reads
    like the C prototype minus the context."""

    def __init__(self, cdll, ctx):
        self._cdll, self._ctx, self._cache = cdll, ctx, {}

    def __getattr__(self, name):
        fn = self._cache.get(name)
        if fn is None:
            raw = getattr(self._cdll, name)            # AttributeError for a missing export, as with the CDLL itself
            if name in NO_CONTEXT:
                fn = raw
            else:
                ctx = self._ctx

                def fn(*args, _raw=raw, _ctx=ctx):
                    return _raw(_ctx, *args)
            self._cache[name] = fn
        return fn


# Test queries added WITHOUT an ABI bump: a library of the same ABI version built before one of them still loads (every kernel entry
# point is there), and calling the missing query raises CvaeError.  The shipped library must export them (__graft_entry__.build and
# tests/test_cabi_exports.py check all of EXPORTS).
ADDITIVE = ("cvae_plan_pass_deep_tiles", "cvae_plan_train_pass", "cvae_stream_move", "cvae_cycle_forward_m2m")
NO_CONTEXT = ("cvae_last_error_string", "cvae_abi_version", "cvae_ctx_create", "cvae_ctx_destroy")
_CDLLS = {}     # path -> (CDLL with argtypes declared): one load per process, any number of contexts


class CvaeLib(object):
    """One CONTEXT (cvae_ctx) of the library: its own status sink, draw origin, options, side stream, profiling brackets.
    gru_vae keeps one per device; new_context() gives another one on the same loaded library."""

    def __init__(self, path=None, _cdll=None):
        path = path or DEFAULT_LIB
        if not os.path.exists(path):
            raise CvaeError("HIP library %s not found: build it with `python __graft_entry__.py` (hipcc "
                            "--offload-arch=gfx950); there is no CPU fallback" % path)
        self.path = path
        if _cdll is None:
            _cdll = _CDLLS.get(path)
        if _cdll is None:
            _cdll = _CDLLS[path] = self._declare(C.CDLL(path), path)
        self.cdll = _cdll
        self.ctx = C.c_void_p(_cdll.cvae_ctx_create())
        if not self.ctx.value:
            raise CvaeError("cvae_ctx_create failed: %s" % _cdll.cvae_last_error_string().decode())
        self.lib = _Bound(_cdll, self.ctx)

    def new_context(self):
        """Another context on the same loaded library (its own options, draw origin, status sink, side stream)."""
        return CvaeLib(self.path, _cdll=self.cdll)

    def close(self):
        """Destroy the context (after the streams it enqueued on have been synchronised)."""
        if getattr(self, "ctx", None) is not None and self.ctx.value:
            self.cdll.cvae_ctx_destroy(self.ctx)
            self.ctx = C.c_void_p(None)

    @staticmethod
    def _declare(L, path):
        L.cvae_last_error_string.restype = C.c_char_p
        L.cvae_abi_version.restype = C.c_int
        for fn in ("cvae_net_prepared_bytes", "cvae_net_prepare_scratch_bytes"):
            getattr(L, fn).restype = C.c_size_t
            getattr(L, fn).argtypes = [C.POINTER(NetDesc)]
        L.cvae_net_prepare.restype = C.c_int
        L.cvae_net_prepare.argtypes = [C.POINTER(NetDesc), C.POINTER(NetWeights), _fp, C.c_size_t, _fp, C.c_size_t, _fp]
        L.cvae_net_prepared_in_range.restype = C.c_int
        L.cvae_net_prepared_in_range.argtypes = [C.POINTER(NetDesc), C.c_int, _fp, _fp]
        L.cvae_pass_workspace_bytes.restype = C.c_size_t
        L.cvae_pass_workspace_bytes.argtypes = [C.POINTER(NetDesc), C.c_int, C.c_int]
        L.cvae_gru_rnn_forward.restype = C.c_int
        L.cvae_gru_rnn_forward.argtypes = [C.POINTER(NetDesc), _fp, C.POINTER(PassInput), _fp, _fp, C.c_int, C.c_int,
                                           C.c_int, _fp, _fp, _fp, _fp, C.c_size_t, C.c_int, _fp]
        L.cvae_gru_rnn_forward_stacked.restype = C.c_int
        L.cvae_gru_rnn_forward_stacked.argtypes = [C.POINTER(NetDesc), _fp, C.c_int, C.POINTER(PassInput), C.POINTER(C.c_void_p),
                                                   C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), _fp, C.c_size_t, C.c_int, _fp]
        L.cvae_gru_rnn_forward_stacked_carry.restype = C.c_int
        L.cvae_gru_rnn_forward_stacked_carry.argtypes = [C.POINTER(NetDesc), _fp, C.c_int, C.POINTER(PassInput), C.POINTER(C.c_void_p),
                                                         C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p),
                                                         C.POINTER(C.c_void_p), _fp, C.c_size_t, C.c_int, _fp]
        for fn in ("cvae_net_prepared_bytes_deep", "cvae_net_prepare_scratch_bytes_deep"):
            getattr(L, fn).restype = C.c_size_t
            getattr(L, fn).argtypes = [C.POINTER(NetDesc), C.c_int]
        L.cvae_net_prepare_deep.restype = C.c_int
        L.cvae_net_prepare_deep.argtypes = [C.POINTER(NetDesc), C.c_int, C.POINTER(NetWeights), C.POINTER(GruLayer), _fp, C.c_size_t, _fp,
                                            C.c_size_t, _fp]
        L.cvae_pass_workspace_bytes_deep.restype = C.c_size_t
        L.cvae_pass_workspace_bytes_deep.argtypes = [C.POINTER(NetDesc), C.c_int, C.c_int, C.c_int]
        L.cvae_plan_pass.restype = C.c_int
        L.cvae_plan_pass.argtypes = [C.POINTER(NetDesc), C.c_int, C.c_int, C.c_int]
        L.cvae_plan_pass_deep.restype = C.c_int
        L.cvae_plan_pass_deep.argtypes = [C.POINTER(NetDesc), C.c_int, C.c_int, C.c_int, C.c_int]
        if hasattr(L, "cvae_plan_pass_deep_tiles"):      # (ADDITIVE, below)
            L.cvae_plan_pass_deep_tiles.restype = C.c_int
            L.cvae_plan_pass_deep_tiles.argtypes = [C.POINTER(NetDesc), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32 * 4)]
        L.cvae_gru_rnn_forward_deep.restype = C.c_int
        L.cvae_gru_rnn_forward_deep.argtypes = [C.POINTER(NetDesc), C.c_int, _fp, C.POINTER(PassInput), _fp, _fp, C.c_int, C.c_int,
                                                C.c_int, _fp, _fp, _fp, _fp, C.c_size_t, C.c_int, _fp]
        L.cvae_sample.restype = C.c_int
        L.cvae_sample.argtypes = [_fp, C.c_int, C.c_int, _fp, C.c_uint64, C.c_uint64, _fp, _fp, _fp]
        L.cvae_sample_laplace.restype = C.c_int
        L.cvae_sample_laplace.argtypes = [_fp, C.c_int, C.c_int, _fp, C.c_uint64, C.c_uint64, _fp, _fp, _fp]
        L.cvae_sample_laplace_backward.restype = C.c_int
        L.cvae_sample_laplace_backward.argtypes = [_fp, _fp, _fp, C.c_int, C.c_int, _fp, _fp]
        L.cvae_cycle_workspace_bytes.restype = C.c_size_t
        L.cvae_cycle_workspace_bytes.argtypes = [C.POINTER(NetDesc), C.POINTER(NetDesc), C.c_int, C.c_int, C.c_int]
        L.cvae_cycle_forward.restype = C.c_int
        L.cvae_cycle_forward.argtypes = [C.POINTER(NetDesc), _fp, C.POINTER(NetDesc), _fp, _fp, _fp, C.c_int, _fp, _fp,
                                         C.c_int, _fp, _fp, C.c_int, C.c_int, C.c_int, C.c_int, _fp, C.c_uint64,
                                         _fp, _fp, _fp, _fp, _fp, _fp, C.c_size_t, C.c_int, _fp]
        L.cvae_cycle_forward_carry.restype = C.c_int
        L.cvae_cycle_forward_carry.argtypes = L.cvae_cycle_forward.argtypes + [C.POINTER(CycleState), C.POINTER(CycleState)]
        if hasattr(L, "cvae_cycle_forward_m2m"):         # (ADDITIVE, below)
            L.cvae_cycle_forward_m2m.restype = C.c_int
            L.cvae_cycle_forward_m2m.argtypes = L.cvae_cycle_forward_carry.argtypes + [C.c_int64, C.c_int64]
        L.cvae_workspace_status.restype = C.c_int
        L.cvae_workspace_status.argtypes = [_fp, C.POINTER(C.c_int32 * 4), _fp]
        L.cvae_train_image_bytes.restype = C.c_size_t
        L.cvae_train_image_bytes.argtypes = [C.POINTER(NetDesc)]
        L.cvae_net_prepare_train.restype = C.c_int
        L.cvae_net_prepare_train.argtypes = [C.POINTER(NetDesc), C.POINTER(NetWeights), _fp, C.c_size_t, C.c_float, _fp]
        L.cvae_net_prepare_train_v.restype = C.c_int
        L.cvae_net_prepare_train_v.argtypes = [C.POINTER(NetDesc), C.POINTER(NetWeights), _fp, C.c_size_t, C.c_float, C.c_int, _fp]
        L.cvae_train_variants_needed.restype = C.c_int
        L.cvae_train_variants_needed.argtypes = [C.POINTER(NetDesc), C.c_int, C.c_int]
        if hasattr(L, "cvae_plan_train_pass"):           # (ADDITIVE, below)
            L.cvae_plan_train_pass.restype = C.c_int
            L.cvae_plan_train_pass.argtypes = [C.POINTER(NetDesc), C.c_int, C.c_int, C.POINTER(C.c_int32 * 12)]
        for fn in ("cvae_train_tape_bytes", "cvae_train_scratch_bytes"):
            getattr(L, fn).restype = C.c_size_t
            getattr(L, fn).argtypes = [C.POINTER(NetDesc), C.c_int, C.c_int]
        L.cvae_gru_rnn_forward_train.restype = C.c_int
        L.cvae_gru_rnn_forward_train.argtypes = [C.POINTER(NetDesc), _fp, _fp, _fp, _fp, C.c_int, C.c_int, C.c_int, _fp, _fp,
                                                 C.c_uint64, C.c_float, _fp, _fp, _fp, _fp, C.c_size_t, _fp, C.c_size_t, _fp]
        L.cvae_gru_rnn_backward.restype = C.c_int
        L.cvae_gru_rnn_backward.argtypes = [C.POINTER(NetDesc), _fp, _fp, C.c_int, C.c_int, C.c_int, _fp, _fp, C.c_size_t, _fp,
                                            C.POINTER(NetGrads), C.c_int, _fp]
        L.cvae_train_debug_counters.restype = C.c_int
        L.cvae_train_debug_counters.argtypes = [C.POINTER(NetDesc), C.c_int, C.c_int, _fp, C.POINTER(C.c_longlong * 8), _fp]
        L.cvae_adam_step.restype = C.c_int
        L.cvae_adam_step.argtypes = [_fp, _fp, _fp, _fp, C.c_size_t, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, _fp, _fp]
        L.cvae_adam_step_counted.restype = C.c_int
        L.cvae_adam_step_counted.argtypes = [_fp, _fp, _fp, _fp, C.c_size_t, C.c_float, C.c_float, C.c_float, C.c_float, _fp, _fp, _fp]
        L.cvae_sample_cat.restype = C.c_int
        L.cvae_sample_cat.argtypes = [_fp, _fp, _fp, _fp, _fp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_int, _fp, _fp, _fp]
        L.cvae_sample_cat_backward.restype = C.c_int
        L.cvae_sample_cat_backward.argtypes = [_fp, _fp, _fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp]
        L.cvae_stage4_loss.restype = C.c_int
        L.cvae_stage4_loss.argtypes = [_fp, _fp, _fp, _fp, _fp, C.c_int, C.c_int, _fp, _fp, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int,
                                       _fp, _fp, _fp, _fp, _fp, _fp, C.c_int, _fp]
        L.cvae_mcd_l1.restype = C.c_int
        L.cvae_mcd_l1.argtypes = [_fp, C.c_long, _fp, C.c_long, C.c_int, C.c_int, _fp, _fp, _fp]
        L.cvae_mcd_l1_backward.restype = C.c_int
        L.cvae_mcd_l1_backward.argtypes = [_fp, C.c_long, _fp, C.c_long, C.c_int, C.c_int, _fp, _fp, _fp, _fp, _fp]
        L.cvae_kl_gauss.restype = C.c_int
        L.cvae_kl_gauss.argtypes = [_fp, C.c_long, C.c_int, C.c_int, _fp, _fp]
        L.cvae_kl_gauss_backward.restype = C.c_int
        L.cvae_kl_gauss_backward.argtypes = [_fp, C.c_long, C.c_int, C.c_int, _fp, _fp, _fp]
        L.cvae_gv_postfilter.restype = C.c_int
        L.cvae_gv_postfilter.argtypes = [_fp, C.c_int, C.c_int, _fp, _fp, _fp, _fp, _fp, _fp, _fp]
        L.cvae_mc2e.restype = C.c_int
        L.cvae_mc2e.argtypes = [_fp, C.c_int, C.c_long, C.c_int, C.c_int, C.c_double, C.c_int, _fp, _fp]
        L.cvae_mcd_aligned.restype = C.c_int
        L.cvae_mcd_aligned.argtypes = [_fp, C.c_long, _fp, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp]
        L.cvae_dtw_work_bytes.restype = C.c_size_t
        L.cvae_dtw_work_bytes.argtypes = [C.c_int, C.c_int]
        L.cvae_dtw_org_to_trg.restype = C.c_int
        L.cvae_dtw_org_to_trg.argtypes = [_fp, _fp, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _fp, _fp, C.c_size_t, _fp]
        L.cvae_dtw_batch_work_bytes.restype = C.c_size_t
        L.cvae_dtw_batch_work_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
        L.cvae_dtw_batch.restype = C.c_int
        L.cvae_dtw_batch.argtypes = [C.POINTER(DtwProblem), C.c_int, _fp, C.c_size_t, _fp]
        L.cvae_eval_stats.restype = C.c_int
        L.cvae_eval_stats.argtypes = [_fp, C.c_int, _fp, _fp]
        L.cvae_latent_mean.restype = C.c_int
        L.cvae_latent_mean.argtypes = [C.POINTER(LatMeanJob), C.c_int, C.c_int, C.c_int, C.c_uint64, _fp]
        L.cvae_mc2e_batch_work_bytes.restype = C.c_size_t
        L.cvae_mc2e_batch_work_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
        L.cvae_mc2e_batch.restype = C.c_int
        L.cvae_mc2e_batch.argtypes = [C.POINTER(Mc2eJob), C.c_int, C.c_double, C.c_int, _fp, C.c_size_t, _fp]
        L.cvae_decode_jobs.restype = C.c_int
        L.cvae_decode_jobs.argtypes = [C.POINTER(DecodeJob), C.c_int, _fp, C.c_size_t, _fp]
        L.cvae_trainlog_window.restype = C.c_int
        L.cvae_trainlog_window.argtypes = [C.POINTER(TrainlogWindowArgs), _fp]
        if hasattr(L, "cvae_stream_move"):               # (ADDITIVE, below)
            L.cvae_stream_move.restype = C.c_int
            L.cvae_stream_move.argtypes = [C.POINTER(MoveJob), C.c_int, _fp]
        L.cvae_step_timing.restype = C.c_int
        L.cvae_step_timing.argtypes = [C.POINTER(NetDesc), C.c_int, C.c_int, _fp, C.POINTER(C.c_double * 8), _fp]
        L.cvae_profile_collect.restype = C.c_int
        L.cvae_profile_collect.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_int)]
        L.cvae_profile_collect_launches.restype = C.c_int
        L.cvae_profile_collect_launches.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]
        L.cvae_train_profile_collect.restype = C.c_int
        L.cvae_train_profile_collect.argtypes = [C.POINTER(C.c_double * 4), C.POINTER(C.c_int * 4), C.POINTER(C.c_double * 4)]
        L.cvae_set_status_sink.restype = C.c_int
        L.cvae_set_status_sink.argtypes = [_fp]
        L.cvae_status_latch.restype = C.c_int
        L.cvae_status_latch.argtypes = [_fp, _fp]
        L.cvae_set_draw_origin.restype = C.c_int
        L.cvae_set_draw_origin.argtypes = [C.c_int64, C.c_int64, C.c_int64]
        L.cvae_set_side_stream.restype = C.c_int
        L.cvae_set_side_stream.argtypes = [C.c_void_p]
        L.cvae_join_side_stream.restype = C.c_int
        L.cvae_join_side_stream.argtypes = [C.c_void_p]
        L.cvae_selftest_limbs.restype = C.c_int
        L.cvae_selftest_limbs.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.cvae_selftest_occupy.restype = C.c_int
        L.cvae_selftest_occupy.argtypes = [C.c_int, C.c_size_t, C.c_int64, C.c_void_p]
        L.cvae_selftest_gemm_work_bytes.restype = C.c_size_t
        L.cvae_selftest_gemm_work_bytes.argtypes = []
        L.cvae_selftest_gemm.restype = C.c_int
        L.cvae_selftest_gemm.argtypes = [C.POINTER(GemmCase), _fp, C.c_size_t, C.POINTER(C.c_int32 * 4), _fp]
        L.cvae_set_draw_parts.restype = C.c_int
        L.cvae_set_draw_parts.argtypes = [C.c_int32]
        L.cvae_set_option.restype = C.c_int
        L.cvae_set_option.argtypes = [C.c_char_p, C.c_int64]
        L.cvae_get_option.restype = C.c_int
        L.cvae_get_option.argtypes = [C.c_char_p, C.POINTER(C.c_int64)]
        L.cvae_reset_options.restype = C.c_int
        L.cvae_reset_options.argtypes = []
        v = L.cvae_abi_version()
        if v != ABI_VERSION:
            raise CvaeError("%s has ABI version %d, binding expects %d" % (path, v, ABI_VERSION))
        # ABI 6: the context handle in front of every other argument
        L.cvae_ctx_create.restype = C.c_void_p
        L.cvae_ctx_create.argtypes = []
        L.cvae_ctx_destroy.restype = C.c_int
        L.cvae_ctx_destroy.argtypes = [C.c_void_p]
        for name in EXPORTS:
            if name not in NO_CONTEXT and (name not in ADDITIVE or hasattr(L, name)):
                fn = getattr(L, name)
                fn.argtypes = [C.c_void_p] + list(fn.argtypes or [])
        return L

    # -- helpers ------------------------------------------------------------------------------------
    def _check(self, rc, what):
        if rc != 0:
            raise CvaeError("%s failed (%d): %s" % (what, rc, self.lib.cvae_last_error_string().decode()))

    @staticmethod
    def desc(in_dim, out_dim, hidden, kernel_size=3, layers=2, has_scale_in=False, has_scale_out=False):
        return NetDesc(in_dim, out_dim, hidden, kernel_size, layers, int(bool(has_scale_in)), int(bool(has_scale_out)))

    # -- entry points -------------------------------------------------------------------------------
    def prepared_bytes(self, d):
        n = self.lib.cvae_net_prepared_bytes(C.byref(d))
        if n == 0:
            raise CvaeError("bad net descriptor: %s" % self.lib.cvae_last_error_string().decode())
        return n

    def prepare_scratch_bytes(self, d):
        return self.lib.cvae_net_prepare_scratch_bytes(C.byref(d))

    def net_prepare(self, d, weight_ptrs, prepared, prepared_bytes, scratch, scratch_bytes, stream=0):
        w = NetWeights(**{f: weight_ptrs.get(f) or None for f in WEIGHT_FIELDS})
        self._check(self.lib.cvae_net_prepare(C.byref(d), C.byref(w), prepared, prepared_bytes, scratch, scratch_bytes,
                                              stream or None), "cvae_net_prepare")

    def net_prepared_in_range(self, d, n_layers, prepared, stream=0):
        """True when the folded weights of a prepared image fit the fp16 limb images (ABI 8; synchronises `stream`).  The context
        remembers a False by the image's address and runs that image's passes on the fp32-operand kernels."""
        rc = self.lib.cvae_net_prepared_in_range(C.byref(d), n_layers, prepared, stream or None)
        if rc < 0:
            self._check(rc, "cvae_net_prepared_in_range")
        return rc == 1

    def pass_workspace_bytes(self, d, B, T):
        n = self.lib.cvae_pass_workspace_bytes(C.byref(d), B, T)
        if n == 0:
            raise CvaeError("cvae_pass_workspace_bytes: bad arguments (B=%d, T=%d)" % (B, T))
        return n

    @staticmethod
    def pass_input(seg0, seg1=None, lat=None, lat_dim=0, eps=None, seed=0, draw_id=0, frames=0, n_draws=0, ctx_before=0, ctx_after=0,
                   draw_frame0=0, eps_draw_stride=0):
        """seg = (ptr, width, row_stride).  ctx_* / draw_frame0 / eps_draw_stride: the input is a window of a longer utterance
        (cvae_pass_input, ABI 5)."""
        s0 = Seg(seg0[0], seg0[1], seg0[2])
        s1 = Seg(seg1[0], seg1[1], seg1[2]) if seg1 else Seg(None, 0, 0)
        return PassInput(s0, s1, lat or None, lat_dim, eps or None, seed, draw_id, frames, n_draws, ctx_before, ctx_after, draw_frame0,
                         eps_draw_stride)

    def gru_rnn_forward_stacked(self, d, prepared, pins, y_ins, B, T, clamp_lat_dim, trj_outs, ws, ws_bytes, flags=0, stream=0):
        n = len(pins)
        arr = (PassInput * n)(*pins)
        ys = (C.c_void_p * n)(*y_ins)
        outs = (C.c_void_p * n)(*trj_outs)
        self._check(self.lib.cvae_gru_rnn_forward_stacked(C.byref(d), prepared, n, arr, ys, B, T, clamp_lat_dim, outs, ws,
                                                          ws_bytes, flags, stream or None), "cvae_gru_rnn_forward_stacked")

    def gru_rnn_forward_stacked_carry(self, d, prepared, pins, y_ins, h_ins, B, T, clamp_lat_dim, trj_outs, h_lasts, ws, ws_bytes,
                                      flags=0, stream=0):
        """y_ins[c] None with h_ins[c] set: the window continues the recurrence that left h_ins[c]."""
        n = len(pins)
        arr = (PassInput * n)(*pins)
        ys = (C.c_void_p * n)(*[y or None for y in y_ins])
        hi = (C.c_void_p * n)(*[h or None for h in h_ins])
        outs = (C.c_void_p * n)(*trj_outs)
        hl = (C.c_void_p * n)(*[h or None for h in h_lasts])
        self._check(self.lib.cvae_gru_rnn_forward_stacked_carry(C.byref(d), prepared, n, arr, ys, hi, B, T, clamp_lat_dim, outs, hl,
                                                                ws, ws_bytes, flags, stream or None),
                    "cvae_gru_rnn_forward_stacked_carry")

    def gru_rnn_forward(self, d, prepared, pin, y_in, h_in, B, T, clamp_lat_dim, trj_out, y_last, h_last, ws, ws_bytes,
                        flags=0, stream=0):
        self._check(self.lib.cvae_gru_rnn_forward(C.byref(d), prepared, C.byref(pin), y_in, h_in or None, B, T,
                                                  clamp_lat_dim, trj_out, y_last or None, h_last or None, ws, ws_bytes,
                                                  flags, stream or None), "cvae_gru_rnn_forward")

    # -- networks with n_layers >= 2 GRU layers (ABI 7; n_layers == 1: the one-layer entry points under another name) ----
    def prepared_bytes_deep(self, d, n_layers):
        n = self.lib.cvae_net_prepared_bytes_deep(C.byref(d), n_layers)
        if n == 0:
            raise CvaeError("bad net descriptor / n_layers: %s" % self.lib.cvae_last_error_string().decode())
        return n

    def prepare_scratch_bytes_deep(self, d, n_layers):
        return self.lib.cvae_net_prepare_scratch_bytes_deep(C.byref(d), n_layers)

    def net_prepare_deep(self, d, n_layers, weight_ptrs, upper_ptrs, prepared, prepared_bytes, scratch, scratch_bytes, stream=0):
        """upper_ptrs: one (w_ih, w_hh, b_ih, b_hh) tuple of device addresses per GRU layer 1 .. n_layers-1."""
        if len(upper_ptrs) != n_layers - 1:
            raise CvaeError("net_prepare_deep: %d upper layers given, n_layers=%d" % (len(upper_ptrs), n_layers))
        w = NetWeights(**{f: weight_ptrs.get(f) or None for f in WEIGHT_FIELDS})
        up = (GruLayer * max(1, n_layers - 1))(*[GruLayer(*u) for u in upper_ptrs])
        self._check(self.lib.cvae_net_prepare_deep(C.byref(d), n_layers, C.byref(w), up, prepared, prepared_bytes, scratch,
                                                   scratch_bytes, stream or None), "cvae_net_prepare_deep")

    def pass_workspace_bytes_deep(self, d, n_layers, B, T):
        n = self.lib.cvae_pass_workspace_bytes_deep(C.byref(d), n_layers, B, T)
        if n == 0:
            raise CvaeError("cvae_pass_workspace_bytes_deep: bad arguments (n_layers=%d, B=%d, T=%d)" % (n_layers, B, T))
        return n

    def plan_pass(self, d, rows, T, flags=0):
        """EVAL_PER_STEP .. EVAL_V6H: the recurrence a one-layer eval pass of `rows` batch rows in all takes."""
        rc = self.lib.cvae_plan_pass(C.byref(d), rows, T, flags)
        if rc < 0:
            self._check(rc, "cvae_plan_pass")
        return rc

    def plan_pass_deep(self, d, n_layers, B, T, flags=0):
        """DEEP_PER_STEP / DEEP_GENERIC / DEEP_RESIDENT: the recurrence a pass of this shape takes."""
        rc = self.lib.cvae_plan_pass_deep(C.byref(d), n_layers, B, T, flags)
        if rc < 0:
            self._check(rc, "cvae_plan_pass_deep")
        return rc

    def plan_pass_deep_tiles(self, d, n_layers, B, T, flags=0):
        """[path, Bp, rts, tiles]: the whole plan cvae_plan_pass_deep reports the path of (tiles: the most row tiles one block handles
        per frame -- 32-row tiles on the resident kernel, 16-row tiles on the any-H kernel)."""
        if not hasattr(self.lib, "cvae_plan_pass_deep_tiles"):
            raise CvaeError("%s was built before cvae_plan_pass_deep_tiles was added: rebuild it" % self.path)
        out = (C.c_int32 * 4)()
        self._check(self.lib.cvae_plan_pass_deep_tiles(C.byref(d), n_layers, B, T, flags, C.byref(out)), "cvae_plan_pass_deep_tiles")
        return list(out)

    def gru_rnn_forward_deep(self, d, n_layers, prepared, pin, y_in, h_in, B, T, clamp_lat_dim, trj_out, y_last, h_last, ws, ws_bytes,
                             flags=0, stream=0):
        """h_in / h_last: [n_layers][B][H] device addresses or None."""
        self._check(self.lib.cvae_gru_rnn_forward_deep(C.byref(d), n_layers, prepared, C.byref(pin), y_in, h_in or None, B, T,
                                                       clamp_lat_dim, trj_out, y_last or None, h_last or None, ws, ws_bytes, flags,
                                                       stream or None), "cvae_gru_rnn_forward_deep")

    def sample(self, lat, rows, lat_dim, eps, seed, draw_id, z, eps_out=None, stream=0):
        self._check(self.lib.cvae_sample(lat, rows, lat_dim, eps or None, seed, draw_id, z, eps_out or None,
                                         stream or None), "cvae_sample")

    def sample_laplace(self, lat, rows, lat_dim, eps, seed, draw_id, z, eps_out=None, stream=0):
        self._check(self.lib.cvae_sample_laplace(lat, rows, lat_dim, eps or None, seed, draw_id, z, eps_out or None, stream or None),
                    "cvae_sample_laplace")

    def sample_laplace_backward(self, dz, lat, z, rows, lat_dim, dlat, stream=0):
        self._check(self.lib.cvae_sample_laplace_backward(dz, lat, z, rows, lat_dim, dlat, stream or None), "cvae_sample_laplace_backward")

    def cycle_workspace_bytes(self, de, dd, B, T, n_cyc):
        n = self.lib.cvae_cycle_workspace_bytes(C.byref(de), C.byref(dd), B, T, n_cyc)
        if n == 0:
            raise CvaeError("cvae_cycle_workspace_bytes: bad arguments")
        return n

    def cycle_forward(self, de, enc_prep, dd, dec_prep, x, cvx, stdim, code_src, code_trg, ncode, y_in_enc, y_in_dec,
                      B, T, n_cyc, lat_dim, eps, seed, out_lat, out_rec, out_cv, out_latcv, out_reccyc, ws, ws_bytes,
                      flags=0, stream=0):
        self._check(self.lib.cvae_cycle_forward(C.byref(de), enc_prep, C.byref(dd), dec_prep, x, cvx, stdim, code_src,
                                                code_trg, ncode, y_in_enc, y_in_dec, B, T, n_cyc, lat_dim, eps or None,
                                                seed, out_lat or None, out_rec or None, out_cv or None,
                                                out_latcv or None, out_reccyc or None, ws, ws_bytes, flags,
                                                stream or None), "cvae_cycle_forward")

    def cycle_forward_carry(self, de, enc_prep, dd, dec_prep, x, cvx, stdim, code_src, code_trg, ncode, y_in_enc, y_in_dec,
                            B, T, n_cyc, lat_dim, eps, seed, out_lat, out_rec, out_cv, out_latcv, out_reccyc, ws, ws_bytes,
                            flags=0, stream=0, state_in=None, state_out=None):
        """state_in / state_out: None or (y_enc, y_dec, h_enc, h_dec) device pointers (cvae_cycle_state)."""
        si = CycleState(*state_in) if state_in else None
        so = CycleState(*state_out) if state_out else None
        self._check(self.lib.cvae_cycle_forward_carry(C.byref(de), enc_prep, C.byref(dd), dec_prep, x, cvx, stdim, code_src,
                                                      code_trg, ncode, y_in_enc, y_in_dec, B, T, n_cyc, lat_dim, eps or None,
                                                      seed, out_lat or None, out_rec or None, out_cv or None,
                                                      out_latcv or None, out_reccyc or None, ws, ws_bytes, flags,
                                                      stream or None, C.byref(si) if si else None, C.byref(so) if so else None),
                    "cvae_cycle_forward_carry")

    def cycle_forward_m2m(self, de, enc_prep, dd, dec_prep, x, cvx, stdim, code_src, code_trg, ncode, y_in_enc, y_in_dec,
                          B, T, n_cyc, lat_dim, eps, seed, out_lat, out_rec, out_cv, out_latcv, out_reccyc, ws, ws_bytes,
                          flags=0, stream=0, state_in=None, state_out=None, cvx_cycle_stride=0, code_trg_cycle_stride=0):
        """cycle_forward_carry with per-cycle cvx [n_cyc,B,T,stdim] / code_trg [n_cyc,B,T,ncode]: the strides are in elements, 0 = one
        tensor for every cycle.  state_in / state_out None: the fresh form."""
        si = CycleState(*state_in) if state_in else None
        so = CycleState(*state_out) if state_out else None
        self._check(self.lib.cvae_cycle_forward_m2m(C.byref(de), enc_prep, C.byref(dd), dec_prep, x, cvx, stdim, code_src,
                                                    code_trg, ncode, y_in_enc, y_in_dec, B, T, n_cyc, lat_dim, eps or None,
                                                    seed, out_lat or None, out_rec or None, out_cv or None,
                                                    out_latcv or None, out_reccyc or None, ws, ws_bytes, flags,
                                                    stream or None, C.byref(si) if si else None, C.byref(so) if so else None,
                                                    int(cvx_cycle_stride), int(code_trg_cycle_stride)),
                    "cvae_cycle_forward_m2m")

    # -- training ------------------------------------------------------------------------------------
    def train_image_bytes(self, d):
        return self.lib.cvae_train_image_bytes(C.byref(d))

    def net_prepare_train(self, d, weight_ptrs, image, image_bytes, stream=0, gru_drop_p=0.0, variants=7):
        """variants: OR of 1 (exact-operand tile kernels), 2 (fp16-pair kernels), 4 (fp32-MFMA forward): the MFMA-order images to build."""
        w = NetWeights(**{f: weight_ptrs.get(f) or None for f in WEIGHT_FIELDS})
        self._check(self.lib.cvae_net_prepare_train_v(C.byref(d), C.byref(w), image, image_bytes, gru_drop_p, int(variants),
                                                      stream or None), "cvae_net_prepare_train_v")

    def train_variants_needed(self, d, B, T):
        return self.lib.cvae_train_variants_needed(C.byref(d), B, T)

    def plan_train_pass(self, d, B, T):
        """dict of TRAIN_PLAN_FIELDS: the recurrence forms (TRAIN_FWD_* / TRAIN_BWD_*) and row tiling a train-mode pass of this shape
        takes under the context's options, and the two memset decisions that follow from them."""
        if not hasattr(self.lib, "cvae_plan_train_pass"):
            raise CvaeError("%s was built before cvae_plan_train_pass was added: rebuild it" % self.path)
        out = (C.c_int32 * 12)()
        self._check(self.lib.cvae_plan_train_pass(C.byref(d), B, T, C.byref(out)), "cvae_plan_train_pass")
        return dict(zip(TRAIN_PLAN_FIELDS, out))

    def train_tape_bytes(self, d, B, T):
        return self.lib.cvae_train_tape_bytes(C.byref(d), B, T)

    def train_scratch_bytes(self, d, B, T):
        return self.lib.cvae_train_scratch_bytes(C.byref(d), B, T)

    def forward_train(self, d, image, x, y_in, h_in, B, T, clamp_lat_dim, cmask, gmask, seed, p_drop, trj_out, y_last, h_last,
                      tape, tape_bytes, scratch, scratch_bytes, stream=0):
        self._check(self.lib.cvae_gru_rnn_forward_train(C.byref(d), image, x, y_in, h_in or None, B, T, clamp_lat_dim,
                                                        cmask or None, gmask or None, seed, p_drop, trj_out, y_last or None,
                                                        h_last or None, tape, tape_bytes, scratch, scratch_bytes,
                                                        stream or None), "cvae_gru_rnn_forward_train")

    def backward(self, d, image, dout, B, T, clamp_lat_dim, tape, scratch, scratch_bytes, dx, grad_ptrs, accumulate=False,
                 stream=0):
        g = NetGrads(**{f: grad_ptrs[f] for f in GRAD_FIELDS})
        self._check(self.lib.cvae_gru_rnn_backward(C.byref(d), image, dout, B, T, clamp_lat_dim, tape, scratch, scratch_bytes,
                                                   dx or None, C.byref(g), int(bool(accumulate)), stream or None),
                    "cvae_gru_rnn_backward")

    def train_debug_counters(self, d, B, T, scratch, stream=0):
        out = (C.c_longlong * 8)()
        self._check(self.lib.cvae_train_debug_counters(C.byref(d), B, T, scratch, C.byref(out), stream or None),
                    "cvae_train_debug_counters")
        return list(out)

    def adam_step(self, p, g, m, v, n, lr, b1, b2, eps, step, stream=0, gate=None):
        self._check(self.lib.cvae_adam_step(p, g, m, v, n, lr, b1, b2, eps, step, gate or None, stream or None), "cvae_adam_step")

    def adam_step_counted(self, p, g, m, v, n, lr, b1, b2, eps, state, stream=0, gate=None):
        self._check(self.lib.cvae_adam_step_counted(p, g, m, v, n, lr, b1, b2, eps, state, gate or None, stream or None),
                    "cvae_adam_step_counted")

    def sample_cat(self, lat, codes, eps, seed, draws, B, T, lat_dim, ncode, out, eps_out, stream=0):
        """codes / eps / draws: one entry per stacked part (1 or 2); eps entries may be None (Philox)."""
        parts = len(codes)
        c = list(codes) + [None] * (2 - parts)
        e = list(eps) + [None] * (2 - parts)
        d = list(draws) + [0] * (2 - parts)
        self._check(self.lib.cvae_sample_cat(lat, c[0], c[1] or None, e[0] or None, e[1] or None, seed, d[0], d[1], B, T, lat_dim, ncode,
                                             parts, out, eps_out, stream or None), "cvae_sample_cat")

    def sample_cat_backward(self, dout, lat, eps, B, T, lat_dim, ncode, parts, dlat, stream=0):
        self._check(self.lib.cvae_sample_cat_backward(dout, lat, eps, B, T, lat_dim, ncode, parts, dlat, stream or None),
                    "cvae_sample_cat_backward")

    def stage4_loss(self, rec, reccyc, lat, latcv, x, x_stride, stdim, w, latcv_w, kl_scale, B, T, D, lat_dim, d_rec, d_reccyc, d_lat,
                    d_latcv, frame_loss, loss, accumulate, stream=0):
        self._check(self.lib.cvae_stage4_loss(rec, reccyc or None, lat, latcv or None, x, x_stride, stdim, w, latcv_w or None, kl_scale,
                                              B, T, D, lat_dim, d_rec, d_reccyc or None, d_lat, d_latcv or None, frame_loss, loss,
                                              int(bool(accumulate)), stream or None), "cvae_stage4_loss")

    def mcd_l1(self, x, sx, y, sy, frames, D, frame_mcd, out3, stream=0):
        self._check(self.lib.cvae_mcd_l1(x, sx, y, sy, frames, D, frame_mcd, out3, stream or None), "cvae_mcd_l1")

    def mcd_l1_backward(self, x, sx, y, sy, frames, D, frame_mcd, out3, g3, dx, stream=0):
        self._check(self.lib.cvae_mcd_l1_backward(x, sx, y, sy, frames, D, frame_mcd, out3, g3, dx, stream or None), "cvae_mcd_l1_backward")

    def kl_gauss(self, param, stride, frames, lat_dim, out1, stream=0):
        self._check(self.lib.cvae_kl_gauss(param, stride, frames, lat_dim, out1, stream or None), "cvae_kl_gauss")

    def kl_gauss_backward(self, param, stride, frames, lat_dim, g1, dparam, stream=0):
        self._check(self.lib.cvae_kl_gauss_backward(param, stride, frames, lat_dim, g1, dparam, stream or None), "cvae_kl_gauss_backward")

    def gv_postfilter(self, c, T, D, dpow, gv_trg, cvgv, out, out_var, work, stream=0):
        self._check(self.lib.cvae_gv_postfilter(c, T, D, dpow or None, gv_trg, cvgv, out, out_var or None, work, stream or None),
                    "cvae_gv_postfilter")

    def mc2e(self, mc, is_f64, ld, T, D, alpha, irlen, e_out, stream=0):
        self._check(self.lib.cvae_mc2e(mc, 1 if is_f64 else 0, ld, T, D, alpha, irlen, e_out, stream or None), "cvae_mc2e")

    def mcd_aligned(self, a, lda, b, ldb, rows, D, d0, l2, frames, stats, stream=0):
        self._check(self.lib.cvae_mcd_aligned(a, lda, b, ldb, rows, D, d0, 1 if l2 else 0, frames, stats or None, stream or None),
                    "cvae_mcd_aligned")

    def dtw_work_bytes(self, T1, T2):
        return self.lib.cvae_dtw_work_bytes(T1, T2)

    def dtw_org_to_trg(self, org, trg, T1, T2, D, mcd, aligned, twf, frames, mean_out, work, work_bytes, stream=0):
        self._check(self.lib.cvae_dtw_org_to_trg(org, trg, T1, T2, D, mcd, aligned, twf, frames, mean_out, work, work_bytes,
                                                 stream or None), "cvae_dtw_org_to_trg")

    def dtw_batch_work_bytes(self, P, T1max, T2max):
        return self.lib.cvae_dtw_batch_work_bytes(P, T1max, T2max)

    def dtw_batch(self, problems, work, work_bytes, stream=0):
        """problems: list of DtwProblem (a host list; the library copies it)."""
        arr = (DtwProblem * len(problems))(*problems)
        self._check(self.lib.cvae_dtw_batch(arr, len(problems), work, work_bytes, stream or None), "cvae_dtw_batch")

    def eval_stats(self, jobs, n, out, stream=0):
        """jobs: DEVICE-visible address of n StatJob descriptors."""
        self._check(self.lib.cvae_eval_stats(jobs, n, out, stream or None), "cvae_eval_stats")

    def latent_mean(self, jobs, lat_dim, n_draws, seed=0, stream=0):
        """jobs: list of LatMeanJob (a host list; the library reads it before it returns)."""
        arr = (LatMeanJob * max(1, len(jobs)))(*jobs)
        self._check(self.lib.cvae_latent_mean(arr, len(jobs), lat_dim, n_draws, seed, stream or None), "cvae_latent_mean")

    def mc2e_batch_work_bytes(self, n_jobs, Dmax, irlen):
        return self.lib.cvae_mc2e_batch_work_bytes(n_jobs, Dmax, irlen)

    def mc2e_batch(self, jobs, alpha, irlen, work, work_bytes, stream=0):
        """jobs: list of Mc2eJob (a host list; the library copies it)."""
        arr = (Mc2eJob * max(1, len(jobs)))(*jobs)
        self._check(self.lib.cvae_mc2e_batch(arr, len(jobs), alpha, irlen, work, work_bytes, stream or None), "cvae_mc2e_batch")

    def decode_jobs(self, jobs, work, work_bytes, stream=0):
        """jobs: list of DecodeJob (a host list; the library copies it into `work`)."""
        arr = (DecodeJob * max(1, len(jobs)))(*jobs)
        self._check(self.lib.cvae_decode_jobs(arr, len(jobs), work, work_bytes, stream or None), "cvae_decode_jobs")

    def trainlog_window(self, args, stream=0):
        """args: a TrainlogWindowArgs; its host arrays are read before the call returns, nothing is waited for."""
        self._check(self.lib.cvae_trainlog_window(C.byref(args), stream or None), "cvae_trainlog_window")

    def stream_move(self, jobs, stream=0):
        """jobs: list of MoveJob (a host list; the table travels in the kernel arguments): every copy in one launch per 96 jobs."""
        if not hasattr(self.lib, "cvae_stream_move"):
            raise CvaeError("%s was built before cvae_stream_move was added: rebuild it" % self.path)
        arr = (MoveJob * max(1, len(jobs)))(*jobs)
        self._check(self.lib.cvae_stream_move(arr, len(jobs), stream or None), "cvae_stream_move")

    def step_timing(self, d, B, T, ws, stream=0):
        out = (C.c_double * 8)()
        self._check(self.lib.cvae_step_timing(C.byref(d), B, T, ws, C.byref(out), stream or None), "cvae_step_timing")
        return list(out)

    def set_status_sink(self, ptr):
        self._check(self.lib.cvae_set_status_sink(ptr or None), "cvae_set_status_sink")

    def status_latch(self, latch, stream=0):
        self._check(self.lib.cvae_status_latch(latch, stream or None), "cvae_status_latch")

    def set_draw_origin(self, row0, global_rows, frames_per_row=0):
        self._check(self.lib.cvae_set_draw_origin(row0, global_rows, frames_per_row), "cvae_set_draw_origin")

    def selftest_limbs(self, x_ptr, y_ptr, n, stream=None):
        self._check(self.lib.cvae_selftest_limbs(x_ptr, y_ptr, n, stream), "cvae_selftest_limbs")

    def selftest_occupy(self, blocks, lds_bytes, cycles, stream=None):
        self._check(self.lib.cvae_selftest_occupy(blocks, lds_bytes, cycles, stream), "cvae_selftest_occupy")

    def selftest_gemm_work_bytes(self):
        return self.lib.cvae_selftest_gemm_work_bytes()

    def selftest_gemm(self, case, work, work_bytes, stream=None):
        """Runs one GemmCase through the training GEMM wrappers; returns [tiled, TM, TN, slices] of what was launched."""
        ran = (C.c_int32 * 4)()
        self._check(self.lib.cvae_selftest_gemm(C.byref(case), work or None, work_bytes, C.byref(ran), stream or None), "cvae_selftest_gemm")
        return list(ran)

    def set_side_stream(self, stream):
        self._check(self.lib.cvae_set_side_stream(stream), "cvae_set_side_stream")

    def join_side_stream(self, stream):
        self._check(self.lib.cvae_join_side_stream(stream), "cvae_join_side_stream")

    def set_draw_parts(self, parts):
        self._check(self.lib.cvae_set_draw_parts(parts), "cvae_set_draw_parts")

    def set_option(self, name, value):
        """Tuning / diagnostic switches by name (include/cyclevae_hip.h lists them); the library reads no environment variable."""
        self._check(self.lib.cvae_set_option(name.encode(), int(value)), "cvae_set_option")

    def get_option(self, name):
        v = C.c_int64(0)
        self._check(self.lib.cvae_get_option(name.encode(), C.byref(v)), "cvae_get_option")
        return v.value

    def reset_options(self):
        self._check(self.lib.cvae_reset_options(), "cvae_reset_options")

    def profile_collect(self):
        ms, n = C.c_double(0.0), C.c_int(0)
        self._check(self.lib.cvae_profile_collect(C.byref(ms), C.byref(n)), "cvae_profile_collect")
        return ms.value, n.value

    def profile_collect_launches(self, cap=4096):
        """[(ms, stacked rows, input channels)] of the eval launches bracketed since the previous collect (FLAG_PROFILE)."""
        ms, rows, cin = (C.c_double * cap)(), (C.c_int * cap)(), (C.c_int * cap)()
        n = self.lib.cvae_profile_collect_launches(ms, rows, cin, cap)
        if n < 0:
            raise CvaeError("cvae_profile_collect_launches failed (%d): %s" % (n, self.lib.cvae_last_error_string().decode()))
        return [(ms[i], rows[i], cin[i]) for i in range(n)]

    TRAIN_PROFILE_CLASSES = ("fwd_recurrence", "bwd_recurrence", "forward_and_dgrad_gemms", "wgrad_gemms")

    def train_profile_collect(self):
        """{class: (summed ms, brackets, summed GEMM flop)} of the launches bracketed since the previous call (option train_profile)."""
        ms, n, fl = (C.c_double * 4)(), (C.c_int * 4)(), (C.c_double * 4)()
        self._check(self.lib.cvae_train_profile_collect(C.byref(ms), C.byref(n), C.byref(fl)), "cvae_train_profile_collect")
        return {name: (ms[i], n[i], fl[i]) for i, name in enumerate(self.TRAIN_PROFILE_CLASSES)}

    def workspace_status(self, ws, stream=0):
        st = (C.c_int32 * 4)()
        self._check(self.lib.cvae_workspace_status(ws, C.byref(st), stream or None), "cvae_workspace_status")
        return list(st)


EXPORTS = ("cvae_last_error_string", "cvae_abi_version", "cvae_ctx_create", "cvae_ctx_destroy", "cvae_set_status_sink", "cvae_status_latch", "cvae_set_draw_origin", "cvae_set_draw_parts",
           "cvae_set_option", "cvae_get_option", "cvae_reset_options", "cvae_selftest_limbs", "cvae_selftest_occupy", "cvae_selftest_gemm_work_bytes", "cvae_selftest_gemm", "cvae_set_side_stream", "cvae_join_side_stream", "cvae_net_prepared_bytes", "cvae_net_prepare_scratch_bytes",
           "cvae_net_prepare", "cvae_pass_workspace_bytes", "cvae_gru_rnn_forward", "cvae_gru_rnn_forward_stacked", "cvae_gru_rnn_forward_stacked_carry", "cvae_sample", "cvae_sample_laplace", "cvae_sample_laplace_backward",
           "cvae_cycle_workspace_bytes", "cvae_cycle_forward", "cvae_cycle_forward_carry", "cvae_cycle_forward_m2m", "cvae_profile_collect", "cvae_profile_collect_launches", "cvae_train_profile_collect", "cvae_step_timing", "cvae_workspace_status",
           "cvae_train_image_bytes", "cvae_net_prepare_train", "cvae_net_prepare_train_v", "cvae_train_variants_needed", "cvae_plan_train_pass", "cvae_train_tape_bytes", "cvae_train_scratch_bytes",
           "cvae_gru_rnn_forward_train", "cvae_gru_rnn_backward", "cvae_adam_step", "cvae_adam_step_counted", "cvae_train_debug_counters",
           "cvae_sample_cat", "cvae_sample_cat_backward", "cvae_stage4_loss", "cvae_mcd_l1", "cvae_mcd_l1_backward", "cvae_kl_gauss",
           "cvae_kl_gauss_backward",
           "cvae_gv_postfilter", "cvae_mcd_aligned", "cvae_mc2e", "cvae_dtw_work_bytes", "cvae_dtw_org_to_trg",
           "cvae_dtw_batch_work_bytes", "cvae_dtw_batch", "cvae_eval_stats", "cvae_latent_mean",
           "cvae_mc2e_batch_work_bytes", "cvae_mc2e_batch", "cvae_decode_jobs", "cvae_trainlog_window", "cvae_stream_move",
           "cvae_net_prepared_bytes_deep", "cvae_net_prepare_scratch_bytes_deep", "cvae_net_prepare_deep", "cvae_pass_workspace_bytes_deep",
           "cvae_plan_pass", "cvae_plan_pass_deep", "cvae_plan_pass_deep_tiles", "cvae_gru_rnn_forward_deep", "cvae_net_prepared_in_range")
