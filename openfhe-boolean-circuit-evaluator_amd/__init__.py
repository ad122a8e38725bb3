"""MI355X-native batched gate-bootstrapping engine behind the reference's BinFHEContext boundary.

Thin ctypes binding over libbce_amd.so (include/bce_gpu.h, include/bce_circuit.h).  The
class and method names mirror what the reference calls on lbcrypto::BinFHEContext
(src/circuit.cpp:88-91,506,800; src/gate.cpp:112,133,172,198-202) so tests read like the
reference's harnesses.  There is no CPU compute fallback: without the HIP extension or a GPU
every compute call raises.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libbce_amd.so")

# enums (include/bce_gpu.h)
TOY, MEDIUM, STD128_AP, STD128_APOPT, STD128, STD128_OPT, STD192, STD192_OPT, STD256, STD256_OPT = range(10)
AP, GINX = 1, 2
OR, AND, NOR, NAND, XOR_FAST, XNOR_FAST = range(6)
XOR = 0x10006   # BCE_XOR (gate byte 6 with bit 16; the bare code 6 is no op): XOR in one bootstrap of ct1 + ct2 (three-level test polynomial); not an OpenFHE gate
OP_NOT, OP_REFRESH, OP_COPY = 16, 17, 18


def PAIR(op, op2):
    """BCE_PAIR: descriptor word for two different gates of OR, AND, NOR, NAND from one blind rotation; the descriptor
    writes op(in0', in1') to slot `out` and op2(in0', in1') to slot `out + 1`"""
    return int(op) | ((int(op2) + 1) << 8)


FRESH, BOOTSTRAPPED = 0, 1
OK, ERR_ARG, ERR_NO_DEVICE, ERR_HIP, ERR_NO_KEYS, ERR_POOL, ERR_UNSUPPORTED, ERR_STATE = range(8)
P_NAMES = ["n", "N", "q", "Q", "qKS", "baseKS", "dKS", "baseG", "dG", "baseR", "dR", "method", "psi"]

PARAMSET_BY_NAME = {"TOY": TOY, "MEDIUM": MEDIUM, "STD128": STD128, "STD128_OPT": STD128_OPT,
                    "STD192": STD192, "STD192_OPT": STD192_OPT}
METHOD_BY_NAME = {"AP": AP, "GINX": GINX}


class BceError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("bce status %d: %s" % (code, msg))
        self.code = code


class GateDesc(C.Structure):
    _fields_ = [("op", C.c_uint32), ("in0", C.c_uint32), ("in1", C.c_uint32),
                ("out", C.c_uint32), ("neg0", C.c_uint32), ("neg1", C.c_uint32)]


BR_KERNEL_NAMES = ["k_blind_rotate (one wave per transform)", "k_blind_rotate_lat<4,2> (split transform, 1 workgroup/CU)",
                   "k_blind_rotate_lat<4,4> (split transform, 2 workgroups/CU)", "k_blind_rotate64 (64-bit modulus)",
                   "k_bootstrap_dag (persistent, dependency-driven, tail fused)",
                   "captured step schedule (bce_plan_run: one hipGraph launch, timed as one)"]
BR_KERNELS = len(BR_KERNEL_NAMES)


class Timing(C.Structure):
    _fields_ = [("blind_rotate_ms", C.c_double), ("tail_ms", C.c_double),
                ("blind_rotate_launches", C.c_uint64), ("bootstraps", C.c_uint64),
                ("br_ms", C.c_double * BR_KERNELS), ("br_launches", C.c_uint64 * BR_KERNELS), ("br_bootstraps", C.c_uint64 * BR_KERNELS),
                ("fused_tail_launches", C.c_uint64)]


class CheckReport(C.Structure):
    _fields_ = [("checked", C.c_uint64), ("mismatches", C.c_uint64), ("repaired", C.c_uint64), ("sum_err", C.c_int64),
                ("sum_sq_err", C.c_uint64), ("max_abs_err", C.c_uint32), ("log_count", C.c_uint32)]


class CheckEntry(C.Structure):
    _fields_ = [("tag", C.c_uint32), ("index", C.c_uint32), ("instance", C.c_uint32), ("slot", C.c_uint32),
                ("err", C.c_int32), ("got", C.c_uint8), ("expect", C.c_uint8), ("pad", C.c_uint8 * 2)]


CHECK_LOG_CAP = 4096


def _report_dict(r, q):
    """counters of a bce_check_report + the measured noise: rms of the phase error and the margin left to a wrong bit"""
    d = {k: int(getattr(r, k)) for k, _ in CheckReport._fields_}
    d["noise_rms"] = (d["sum_sq_err"] / d["checked"]) ** 0.5 if d["checked"] else 0.0
    d["margin"] = q // 8 - d["max_abs_err"]
    return d


ENGINE_SYMBOLS = [
    "bce_ctx_create", "bce_ctx_create_custom", "bce_ctx_destroy", "bce_last_error", "bce_get_params",
    "bce_keygen", "bce_import_keys", "bce_import_keys_eval", "bce_export_bsk_eval", "bce_import_keys_file", "bce_export_keys_file", "bce_bsk_words", "bce_ksk_words", "bce_export_sk", "bce_export_bsk",
    "bce_export_ksk", "bce_pool_reserve", "bce_pool_slots", "bce_lwe_write", "bce_lwe_read",
    "bce_encrypt_bits", "bce_set_encrypt_seed", "bce_decrypt_bits", "bce_eval_gates", "bce_eval_gates_strided", "bce_synchronize",
    "bce_timing_reset", "bce_timing_get", "bce_timing_set_events", "bce_bytes_per_bootstrap", "bce_bytes_per_bootstrap_parts", "bce_forward_transforms_per_step", "bce_forward_units", "bce_forward_mfma", "bce_lazy_arithmetic", "bce_forward_mfma_tables", "bce_launch_capacity", "bce_rccl_available", "bce_rccl_version", "bce_rccl_unique_id", "bce_rccl_init", "bce_rccl_allgather", "bce_rccl_comm_info",
    "bce_rccl_shutdown", "bce_debug_eval_stages", "bce_debug_ntt", "bce_debug_tail", "bce_debug_tail_split",
    "bce_dag_supported", "bce_dag_create", "bce_dag_create_pairs", "bce_dag_run", "bce_dag_destroy", "bce_dag_set_limits", "bce_dag_last_run", "bce_dag_debug_block_task",
    "bce_dag_set_checks", "bce_dag_set_expected",
    "bce_params_derive", "bce_params_derive_set", "bce_dag_launch_choice",
    "bce_plan_create", "bce_plan_run_step", "bce_plan_run", "bce_plan_destroy",
    "bce_check_slots", "bce_plan_set_checks", "bce_plan_set_expected", "bce_check_reset", "bce_check_get",
    "bce_keyset_add", "bce_keyset_select", "bce_keyset_drop", "bce_keyset_count", "bce_keyset_selected",
    "bce_eval_gates_keyed", "bce_plan_create_keyed", "bce_decrypt_bits_keyed",
]

_lib = None


def build(force=False):
    """Compile the extension for gfx950 if needed and return its path."""
    return _build.build(force=force)


def forward_mfma_tables(Q, N=1024, gBits=7, dG=4):
    """Host-built tables of the matrix-pipe forward body (no context, no GPU): (status, dict).  status 1: may be enabled,
    -1: a bound fails for this Q, 0: not this class of parameters (dict is None)."""
    import numpy as np
    L = lib()
    psi, w14, bounds = C.c_uint64(), (C.c_uint32 * 2)(), (C.c_uint64 * 4)()
    M6, Cw, tab = np.zeros((64, 64), np.uint32), np.zeros(64, np.uint32), np.zeros((4, 4, 64, 4), np.uint32)
    st = int(L.bce_forward_mfma_tables(int(Q), int(N), int(gBits), int(dG), C.byref(psi), M6.ctypes.data, Cw.ctypes.data, tab.ctypes.data,
                                       C.cast(w14, C.c_void_p), C.cast(bounds, C.c_void_p)))
    if st == 0:
        return 0, None
    return st, {"psi": int(psi.value), "M6": M6, "C": Cw, "table": tab, "w14": (int(w14[0]), int(w14[1])),
                "limb_sum_max": int(bounds[0]), "lo_max": int(bounds[1]), "hi_max": int(bounds[2]), "out_max": int(bounds[3])}


def lib():
    """Load libbce_amd.so; raises (never falls back) when the extension is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libbce_amd.so is not built: run `python -m openfhe-boolean-circuit-evaluator_amd.build` "
                          "or __graft_entry__.build(); there is no fallback path")
    L = C.CDLL(LIB_PATH)
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
    L.bce_ctx_create.argtypes = [i32, i32, i32, C.POINTER(vp)]
    L.bce_ctx_create_custom.argtypes = [u32, u32, u64, u64, u64, u32, u32, u32, i32, i32, C.POINTER(vp)]
    L.bce_ctx_destroy.argtypes = [vp]
    L.bce_ctx_destroy.restype = None
    L.bce_last_error.argtypes = [vp]
    L.bce_last_error.restype = C.c_char_p
    L.bce_get_params.argtypes = [vp, C.POINTER(u64)]
    L.bce_keygen.argtypes = [vp, C.c_char_p]
    L.bce_import_keys.argtypes = [vp, vp, vp, vp, u64, vp, u64]
    L.bce_import_keys_eval.argtypes = [vp, vp, vp, vp, u64, vp, u64]
    L.bce_export_bsk_eval.argtypes = [vp, vp]
    L.bce_import_keys_file.argtypes = [vp, C.c_char_p]
    L.bce_export_keys_file.argtypes = [vp, C.c_char_p]
    L.bce_bsk_words.argtypes = [vp]
    L.bce_bsk_words.restype = u64
    L.bce_ksk_words.argtypes = [vp]
    L.bce_ksk_words.restype = u64
    L.bce_export_sk.argtypes = [vp, vp, vp]
    L.bce_export_bsk.argtypes = [vp, vp]
    L.bce_export_ksk.argtypes = [vp, vp]
    L.bce_pool_reserve.argtypes = [vp, u32]
    L.bce_pool_slots.argtypes = [vp]
    L.bce_pool_slots.restype = u32
    L.bce_lwe_write.argtypes = [vp, vp, u32, vp]
    L.bce_lwe_read.argtypes = [vp, vp, u32, vp]
    L.bce_encrypt_bits.argtypes = [vp, vp, vp, u32, u64, i32]
    L.bce_set_encrypt_seed.argtypes = [vp, C.c_char_p]
    L.bce_decrypt_bits.argtypes = [vp, vp, u32, vp]
    L.bce_eval_gates.argtypes = [vp, u32, vp]
    L.bce_eval_gates_strided.argtypes = [vp, u32, vp, u32, u32]
    L.bce_eval_gates_keyed.argtypes = [vp, u32, vp, u32, u32, vp]
    L.bce_decrypt_bits_keyed.argtypes = [vp, vp, u32, vp, vp]
    L.bce_keyset_add.argtypes = [vp, C.POINTER(u32)]
    L.bce_keyset_select.argtypes = [vp, u32]
    L.bce_keyset_drop.argtypes = [vp, u32]
    L.bce_keyset_count.argtypes = [vp]
    L.bce_keyset_count.restype = u32
    L.bce_keyset_selected.argtypes = [vp]
    L.bce_keyset_selected.restype = u32
    L.bce_synchronize.argtypes = [vp]
    L.bce_timing_reset.argtypes = [vp]
    L.bce_timing_get.argtypes = [vp, C.POINTER(Timing)]
    L.bce_timing_set_events.argtypes = [vp, i32]
    L.bce_bytes_per_bootstrap.argtypes = [vp]
    L.bce_bytes_per_bootstrap.restype = u64
    L.bce_bytes_per_bootstrap_parts.argtypes = [vp, C.POINTER(u64)]
    L.bce_forward_transforms_per_step.argtypes = [vp]
    L.bce_forward_transforms_per_step.restype = C.c_uint32
    L.bce_forward_units.argtypes = [vp]
    L.bce_forward_units.restype = C.c_uint32
    L.bce_forward_mfma.argtypes = [vp]
    L.bce_forward_mfma.restype = C.c_uint32
    L.bce_lazy_arithmetic.argtypes = [vp]
    L.bce_lazy_arithmetic.restype = C.c_uint32
    L.bce_forward_mfma_tables.argtypes = [u64, u32, u32, u32, vp, vp, vp, vp, vp, vp]
    L.bce_forward_mfma_tables.restype = i32
    L.bce_launch_capacity.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.bce_rccl_unique_id.argtypes = [C.c_char_p]
    L.bce_rccl_init.argtypes = [vp, C.c_char_p, i32, i32]
    L.bce_rccl_allgather.argtypes = [vp, vp, vp, u64]
    L.bce_rccl_shutdown.argtypes = [vp]
    L.bce_rccl_comm_info.argtypes = [vp, C.POINTER(C.c_int)]
    L.bce_debug_eval_stages.argtypes = [vp, u32, vp, vp, vp, vp]
    L.bce_debug_ntt.argtypes = [vp, vp, u32, i32]
    L.bce_debug_tail.argtypes = [vp, u32, vp, vp, vp, vp]
    L.bce_debug_tail_split.argtypes = [vp, u32]
    L.bce_debug_tail_split.restype = C.c_uint32
    L.bce_dag_supported.argtypes = [vp]
    L.bce_dag_create.argtypes = [vp, u32, vp, vp, C.POINTER(vp)]
    L.bce_dag_create_pairs.argtypes = [vp, u32, vp, vp, C.POINTER(vp)]
    L.bce_dag_run.argtypes = [vp, vp, u32, u32, u32]
    L.bce_dag_destroy.argtypes = [vp, vp]
    L.bce_dag_destroy.restype = None
    L.bce_dag_set_limits.argtypes = [vp, i32, i32, u32, u32]
    L.bce_dag_last_run.argtypes = [vp, C.POINTER(u64)]
    L.bce_dag_debug_block_task.argtypes = [vp, u32]
    L.bce_dag_set_checks.argtypes = [vp, vp, u32, vp, i32]
    L.bce_dag_set_expected.argtypes = [vp, vp, u32, vp]
    L.bce_plan_create.argtypes = [vp, u32, vp, vp, u32, u32, u32, C.POINTER(vp)]
    L.bce_plan_create_keyed.argtypes = [vp, u32, vp, vp, u32, u32, u32, vp, C.POINTER(vp)]
    L.bce_plan_run_step.argtypes = [vp, vp, u32]
    L.bce_plan_run.argtypes = [vp, vp]
    L.bce_plan_destroy.argtypes = [vp, vp]
    L.bce_plan_destroy.restype = None
    L.bce_check_slots.argtypes = [vp, u32, vp, vp, u32, u32, i32, u32]
    L.bce_plan_set_checks.argtypes = [vp, vp, vp, vp, i32]
    L.bce_plan_set_expected.argtypes = [vp, vp, vp]
    L.bce_check_reset.argtypes = [vp]
    L.bce_check_get.argtypes = [vp, C.POINTER(CheckReport), C.POINTER(CheckEntry), u32]
    L.bce_params_derive.argtypes = [u32, u32, u64, u64, u64, u32, u32, u32, i32, u32, C.POINTER(u64), C.POINTER(C.c_char_p)]
    L.bce_params_derive_set.argtypes = [i32, i32, u32, C.POINTER(u64), C.POINTER(C.c_char_p)]
    L.bce_dag_launch_choice.argtypes = [C.POINTER(u64), i32, i32, u32, u32, u32, u64, C.POINTER(u64)]
    _lib = L
    return L


# enum BCE_D_* / BCE_L_* of include/bce_gpu.h
D_NAMES = ["n", "N", "logN", "q", "Q", "qKS", "baseKS", "dKS", "ksk_stride", "ksk_u16", "ks_chunk", "gBits", "dG", "baseR", "dR",
           "method_ap", "factor", "Q8p1", "red_shift", "red_mu", "Ninv", "Ninv_s", "Winv_last", "Winv_last_s", "mu32", "lazy", "c32",
           "occupancy_target", "variant", "cu_count", "xcd_gate_ticks", "fuse_tail", "fold_ninv", "fold", "fwd_units", "factor_even",
           "I4_0", "I4_1", "I4_2", "I4_3", "I4s_0", "I4s_1", "I4s_2", "I4s_3", "qinv_neg", "r2_off", "is64", "Q64", "Q8p1_64", "mu64",
           "c64", "Ninv64", "Ninv64_s", "fp64", "Qd", "invQd", "Ninvd", "Ninvd_q", "pool_stride", "fwd_mfma", "w14", "w14s",
           "xcd_gate", "psi", "family", "fold_build", "dag", "wg_per_cu_lone", "wg_per_cu_full", "lds_bytes",
           "capacity_lone", "capacity_full", "bytes_bsk", "bytes_ksk", "bytes_ct", "forward_transforms",
           "fnv_twf", "fnv_psi", "fnv_psi_r2", "fnv_tw64", "fnv_tw64d", "fnv_fwd_mfma", "dag_lds_bytes"]
L_NAMES = ["wps", "grid", "policy", "gate_ticks", "gate_backlog", "lazy_ticks", "stall_ticks", "rearm_only"]


def derive_params(paramset=None, method=GINX, cu_count=256, custom=None):
    """What a context of this shape would decide about itself, for `cu_count` compute units and the context knobs of the
    environment; no context, no GPU.  custom = (n, N, q, Q, qKS, baseKS, baseG, baseR) instead of a tabulated set.  Returns
    {"status", "message"} and, for status OK, every value of enum BCE_D_* by name (doubles as bit patterns)."""
    L = lib()
    out, msg = (C.c_uint64 * len(D_NAMES))(), C.c_char_p()
    if custom is not None:
        rc = L.bce_params_derive(*[int(v) for v in custom], method, cu_count, out, C.byref(msg))
    else:
        rc = L.bce_params_derive_set(paramset, method, cu_count, out, C.byref(msg))
    d = {"status": int(rc), "message": (msg.value or b"").decode()}
    if rc == OK:
        d.update(zip(D_NAMES, [int(v) for v in out]))
    return d


def dag_launch_choice(derived, depth, items, workgroups_per_cu=0, placement=1, lazy_us=20, stall_ms=4000):
    """What bce_dag_run would launch for a context that derive_params() describes, under the DAG knobs of the environment."""
    L = lib()
    rep, out = (C.c_uint64 * len(D_NAMES))(*[derived[k] for k in D_NAMES]), (C.c_uint64 * len(L_NAMES))()
    rc = L.bce_dag_launch_choice(rep, workgroups_per_cu, placement, lazy_us, stall_ms, depth, items, out)
    if rc != OK:
        raise BceError(rc, "bce_dag_launch_choice")
    return dict(zip(L_NAMES, [int(v) for v in out]))


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def seed_bytes(seed):
    if isinstance(seed, (bytes, bytearray)):
        return bytes(seed).ljust(32, b"\0")[:32]
    return int(seed).to_bytes(32, "little")


def make_descs(descs):
    """list of (op, in0, in1, out[, neg0, neg1]) -> ctypes array of bce_gate_desc"""
    arr = (GateDesc * len(descs))()
    for i, d in enumerate(descs):
        d = tuple(d) + (0,) * (6 - len(d))
        arr[i] = GateDesc(*d)
    return arr


class BinFHEContext:
    """Device-resident equivalent of lbcrypto::BinFHEContext for the calls the reference makes."""

    def __init__(self, paramset=STD128_OPT, method=GINX, device=0, custom=None):
        self._L = lib()
        h = C.c_void_p()
        if custom is not None:
            rc = self._L.bce_ctx_create_custom(*custom, method, device, C.byref(h))
        else:
            rc = self._L.bce_ctx_create(paramset, method, device, C.byref(h))
        if rc != OK:
            raise BceError(rc, self._L.bce_last_error(None).decode())
        self.h = h
        buf = (C.c_uint64 * len(P_NAMES))()
        self._L.bce_get_params(self.h, buf)
        self.params = dict(zip(P_NAMES, [int(v) for v in buf]))
        self.n, self.N = self.params["n"], self.params["N"]

    def _ck(self, rc):
        if rc != OK:
            raise BceError(rc, self._L.bce_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self._L.bce_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- KeyGen + BTKeyGen (src/circuit.cpp:90-91) ---
    def KeyGen(self, seed=None):
        """seed=None: keys from OS entropy (the reference's cc.KeyGen()); an explicit seed gives reproducible
        keys (oracle parity tests, one key set replicated on every rank)."""
        self._ck(self._L.bce_keygen(self.h, None if seed is None else seed_bytes(seed)))

    BTKeyGen = KeyGen

    # --- key sets: one per client; a call without a key-set map acts on the selected set (include/bce_gpu.h) ---
    def keyset_add(self):
        """a new, empty key set; returns its id (the lowest free one, >= 1)"""
        out = C.c_uint32()
        self._ck(self._L.bce_keyset_add(self.h, C.byref(out)))
        return int(out.value)

    def keyset_select(self, keyset):
        self._ck(self._L.bce_keyset_select(self.h, int(keyset)))

    def keyset_drop(self, keyset):
        self._ck(self._L.bce_keyset_drop(self.h, int(keyset)))

    def keyset_count(self):
        return int(self._L.bce_keyset_count(self.h))

    def keyset_selected(self):
        return int(self._L.bce_keyset_selected(self.h))

    def import_keys(self, s, z, bsk, ksk):
        s = np.ascontiguousarray(s, dtype=np.int32)
        z = np.ascontiguousarray(z, dtype=np.int32)
        bsk = np.ascontiguousarray(bsk, dtype=np.uint64)
        ksk = np.ascontiguousarray(ksk, dtype=np.uint32)
        self._ck(self._L.bce_import_keys(self.h, _p(s), _p(z), _p(bsk), bsk.size, _p(ksk), ksk.size))

    def import_keys_eval(self, s, z, bsk_eval, ksk):
        """bootstrapping key already in EVALUATION form, OpenFHE's order (bit-reversed CT order, minimal primitive root)"""
        s = np.ascontiguousarray(s, dtype=np.int32)
        z = np.ascontiguousarray(z, dtype=np.int32)
        bsk = np.ascontiguousarray(bsk_eval, dtype=np.uint64)
        ksk = np.ascontiguousarray(ksk, dtype=np.uint32)
        self._ck(self._L.bce_import_keys_eval(self.h, _p(s), _p(z), _p(bsk), bsk.size, _p(ksk), ksk.size))

    def export_bsk_eval(self):
        out = np.zeros(self._L.bce_bsk_words(self.h), dtype=np.uint64)
        self._ck(self._L.bce_export_bsk_eval(self.h, _p(out)))
        return out

    def import_keys_file(self, path):
        """keys written by tools/openfhe_export/export_keys.cpp (format: tools/openfhe_export/bce_keyfile.h)"""
        self._ck(self._L.bce_import_keys_file(self.h, os.fsencode(path)))

    def export_keys_file(self, path):
        self._ck(self._L.bce_export_keys_file(self.h, os.fsencode(path)))

    def export_sk(self):
        s = np.zeros(self.n, dtype=np.int32)
        z = np.zeros(self.N, dtype=np.int32)
        self._ck(self._L.bce_export_sk(self.h, _p(s), _p(z)))
        return s, z

    def export_bsk(self):
        out = np.zeros(self._L.bce_bsk_words(self.h), dtype=np.uint64)
        self._ck(self._L.bce_export_bsk(self.h, _p(out)))
        return out

    def export_ksk(self):
        out = np.zeros(self._L.bce_ksk_words(self.h), dtype=np.uint32)
        self._ck(self._L.bce_export_ksk(self.h, _p(out)))
        return out

    # --- pool ---
    def pool_reserve(self, slots):
        self._ck(self._L.bce_pool_reserve(self.h, int(slots)))

    def lwe_write(self, slots, cts):
        slots = np.ascontiguousarray(slots, dtype=np.uint32)
        cts = np.ascontiguousarray(cts, dtype=np.uint64)
        assert cts.size == slots.size * (self.n + 1)
        self._ck(self._L.bce_lwe_write(self.h, _p(slots), slots.size, _p(cts)))

    def lwe_read(self, slots):
        slots = np.ascontiguousarray(slots, dtype=np.uint32)
        out = np.zeros((slots.size, self.n + 1), dtype=np.uint64)
        self._ck(self._L.bce_lwe_read(self.h, _p(slots), slots.size, _p(out)))
        return out

    def set_encrypt_seed(self, seed):
        """Deterministic encryption streams (parity tests / identical inputs on every rank); None = back to
        OS entropy + the context's own counter (the default)."""
        self._ck(self._L.bce_set_encrypt_seed(self.h, None if seed is None else seed_bytes(seed)))

    # --- Encrypt / Decrypt (src/circuit.cpp:506,800) ---
    def Encrypt(self, bits, slots, enc_index_base=0, mode=FRESH):
        """enc_index_base only matters after set_encrypt_seed(); by default the context numbers its streams itself"""
        bits = np.ascontiguousarray(bits, dtype=np.uint8)
        slots = np.ascontiguousarray(slots, dtype=np.uint32)
        assert bits.size == slots.size
        self._ck(self._L.bce_encrypt_bits(self.h, _p(bits), _p(slots), slots.size, int(enc_index_base), mode))

    def Decrypt(self, slots, keysets=None):
        """keysets: the key set of every slot (bce_decrypt_bits_keyed), or None: all under the selected set"""
        slots = np.ascontiguousarray(slots, dtype=np.uint32)
        out = np.zeros(slots.size, dtype=np.uint8)
        if keysets is not None:
            ids = np.ascontiguousarray(keysets, dtype=np.uint32)
            if ids.size != slots.size:
                raise ValueError("keysets names %d slots, the call has %d" % (ids.size, slots.size))
            self._ck(self._L.bce_decrypt_bits_keyed(self.h, _p(slots), slots.size, _p(ids), _p(out)))
        else:
            self._ck(self._L.bce_decrypt_bits(self.h, _p(slots), slots.size, _p(out)))
        return out

    # --- the hot path: batched EvalBinGate / EvalNOT (src/gate.cpp:112,133,172,198-202) ---
    def EvalGates(self, descs, instances=1, slot_stride=0, keysets=None):
        """keysets: the key set of every instance (bce_eval_gates_keyed), or None: all run under the selected set"""
        arr = descs if isinstance(descs, C.Array) else make_descs(descs)
        if keysets is not None:
            ids = np.ascontiguousarray(keysets, dtype=np.uint32)
            if ids.size != int(instances):
                raise ValueError("keysets names %d instances, the call has %d" % (ids.size, int(instances)))
            self._ck(self._L.bce_eval_gates_keyed(self.h, len(arr), arr, int(instances), int(slot_stride), _p(ids)))
        elif instances == 1:
            self._ck(self._L.bce_eval_gates(self.h, len(arr), arr))
        else:
            self._ck(self._L.bce_eval_gates_strided(self.h, len(arr), arr, instances, slot_stride))

    def EvalBinGate(self, gate, in0, in1, out):
        self.EvalGates([(gate, in0, in1, out)])

    def EvalNOT(self, in0, out):
        self.EvalGates([(OP_NOT, in0, in0, out)])

    def synchronize(self):
        self._ck(self._L.bce_synchronize(self.h))

    def timing_reset(self):
        self._ck(self._L.bce_timing_reset(self.h))

    def timing_set_events(self, on):
        """per-launch HIP events on (default) / off (counters only; nothing between dependent kernels on the device timeline)"""
        self._ck(self._L.bce_timing_set_events(self.h, int(bool(on))))

    def timing(self):
        t = Timing()
        self._ck(self._L.bce_timing_get(self.h, C.byref(t)))
        return {"blind_rotate_ms": t.blind_rotate_ms, "tail_ms": t.tail_ms,
                "blind_rotate_launches": int(t.blind_rotate_launches), "bootstraps": int(t.bootstraps),
                "fused_tail_launches": int(t.fused_tail_launches),
                "by_kernel": [{"kernel": BR_KERNEL_NAMES[k], "ms": t.br_ms[k], "launches": int(t.br_launches[k]),
                               "bootstraps": int(t.br_bootstraps[k])} for k in range(BR_KERNELS)]}

    def bytes_per_bootstrap(self):
        return int(self._L.bce_bytes_per_bootstrap(self.h))

    # --- dependency-driven evaluation: the whole bootstrap DAG in one persistent launch (bce_dag_*) ---
    def dag_supported(self):
        return bool(self._L.bce_dag_supported(self.h))

    def dag_create(self, tasks, prio=None, pairs=False):
        """tasks: (op, in0, in1, out[, neg0, neg1]) in topological order, SSA slots; returns an opaque handle.
        pairs=True (bce_dag_create_pairs): PAIR words are tasks with the two outputs out and out + 1"""
        arr = (GateDesc * len(tasks))()
        for i, t in enumerate(tasks):
            arr[i] = GateDesc(*(tuple(t) + (0, 0))[:6])
        pr = None
        if prio is not None:
            pr = (C.c_uint8 * len(tasks))(*[int(x) for x in prio])
        h = C.c_void_p()
        create = self._L.bce_dag_create_pairs if pairs else self._L.bce_dag_create
        self._ck(create(self.h, len(tasks), arr, pr, C.byref(h)))
        return h

    def dag_run(self, dag, instances=1, slot_stride=0, slot_base=0):
        self._ck(self._L.bce_dag_run(self.h, dag, int(instances), int(slot_stride), int(slot_base)))

    def dag_destroy(self, dag):
        self._L.bce_dag_destroy(self.h, dag)

    def dag_set_limits(self, workgroups_per_cu=0, placement=1, lazy_us=20, stall_ms=4000):
        self._ck(self._L.bce_dag_set_limits(self.h, int(workgroups_per_cu), int(placement), int(lazy_us), int(stall_ms)))

    def dag_last_run(self):
        out = (C.c_uint64 * 7)()
        self._ck(self._L.bce_dag_last_run(self.h, out))
        d = {"done": int(out[0]), "lazy_waits": int(out[1]), "abort": int(out[2]), "workgroups_per_cu": int(out[3]),
             "busy_ticks": int(out[4]), "wait_ticks": int(out[5]), "gate_ticks": int(out[6])}
        if out[0]:
            d["ms_per_bootstrap"] = round(out[4] / out[0] / 1e5, 4)        # 100 MHz ticks
            d["wait_ms_per_bootstrap"] = round(out[5] / out[0] / 1e5, 4)
            d["gate_ms_per_bootstrap"] = round(out[6] / out[0] / 1e5, 4)
        return d

    # --- a whole step schedule resident on the device (bce_plan_*) ---
    def plan_create(self, steps, instances=1, slot_stride=0, slot_base=0, keysets=None):
        """steps: list of frontiers, each a list of (op, in0, in1, out[, neg0, neg1]); returns an opaque handle.
        keysets: the key set of every instance, fixed for the plan's life (bce_plan_create_keyed)"""
        flat = [t for st in steps for t in st]
        arr = (GateDesc * max(1, len(flat)))()
        for i, t in enumerate(flat):
            arr[i] = GateDesc(*(tuple(t) + (0, 0))[:6])
        sizes = (C.c_uint32 * max(1, len(steps)))(*[len(st) for st in steps])
        h = C.c_void_p()
        if keysets is not None:
            ids = np.ascontiguousarray(keysets, dtype=np.uint32)
            if ids.size != int(instances):
                raise ValueError("keysets names %d instances, the plan has %d" % (ids.size, int(instances)))
            self._ck(self._L.bce_plan_create_keyed(self.h, len(steps), sizes, arr, int(instances), int(slot_stride), int(slot_base), _p(ids), C.byref(h)))
            return h
        self._ck(self._L.bce_plan_create(self.h, len(steps), sizes, arr, int(instances), int(slot_stride), int(slot_base), C.byref(h)))
        return h

    def plan_run_step(self, plan, step):
        self._ck(self._L.bce_plan_run_step(self.h, plan, int(step)))

    def plan_run(self, plan):
        """every step's launches as ONE hipGraph launch (captured at the first call)"""
        self._ck(self._L.bce_plan_run(self.h, plan))

    def plan_destroy(self, plan):
        self._L.bce_plan_destroy(self.h, plan)

    # --- verify mode on the device: decrypt, compare, repair (bce_check_*) ---
    def check_slots(self, slots, expect, instances=1, slot_stride=0, repair=False, tag=0):
        """expect[instances][len(slots)]: asynchronous check of slots[i] + k * slot_stride against expect[k][i]"""
        slots = np.ascontiguousarray(slots, dtype=np.uint32)
        expect = np.ascontiguousarray(expect, dtype=np.uint8)
        assert expect.size == slots.size * int(instances)
        self._ck(self._L.bce_check_slots(self.h, slots.size, _p(slots), _p(expect), int(instances), int(slot_stride), int(bool(repair)), int(tag)))

    def plan_set_checks(self, plan, checks, repair=False):
        """checks: per step of the plan, the instance-0 slots to check after it (may be empty)"""
        sizes = np.array([len(st) for st in checks], dtype=np.uint32)
        slots = np.array([s for st in checks for s in st] or [0], dtype=np.uint32)
        self._ck(self._L.bce_plan_set_checks(self.h, plan, _p(sizes), _p(slots), int(bool(repair))))

    def plan_set_expected(self, plan, expect):
        """expect[instances][total checks] of the next run(s)"""
        expect = np.ascontiguousarray(expect, dtype=np.uint8)
        self._ck(self._L.bce_plan_set_expected(self.h, plan, _p(expect)))

    def check_reset(self):
        self._ck(self._L.bce_check_reset(self.h))

    def check_get(self):
        """(report dict incl. noise_rms and margin, log entries as dicts); synchronises"""
        r = CheckReport()
        log = (CheckEntry * CHECK_LOG_CAP)()
        self._ck(self._L.bce_check_get(self.h, C.byref(r), log, CHECK_LOG_CAP))
        keys = ("tag", "index", "instance", "slot", "err", "got", "expect")
        return _report_dict(r, self.params["q"]), [{k: int(getattr(log[i], k)) for k in keys} for i in range(r.log_count)]

    def dag_set_checks(self, dag, tasks, repair=False):
        """tasks: distinct task indices of the DAG; check i decrypts the `out` register of tasks[i] inside the persistent
        kernel, before the task's consumers are released.  An empty list detaches the checks."""
        tasks = np.ascontiguousarray(tasks, dtype=np.uint32).ravel()
        self._ck(self._L.bce_dag_set_checks(self.h, dag, tasks.size, _p(tasks) if tasks.size else None, int(bool(repair))))

    def dag_set_expected(self, dag, expect):
        """expect[instances][n_checks] of the next run(s)"""
        expect = np.ascontiguousarray(expect, dtype=np.uint8)
        assert expect.ndim == 2
        self._ck(self._L.bce_dag_set_expected(self.h, dag, expect.shape[0], _p(expect)))

    def dag_debug_block_task(self, dag, t):
        self._ck(self._L.bce_dag_debug_block_task(dag, int(t)))

    # --- in-library RCCL all-gather on the engine stream (multi-GPU exchange without host sync) ---
    @staticmethod
    def rccl_available():
        return bool(lib().bce_rccl_available())

    @staticmethod
    def rccl_unique_id():
        buf = C.create_string_buffer(128)
        rc = lib().bce_rccl_unique_id(buf)
        if rc != OK:
            raise BceError(rc, "RCCL is not available (bce_rccl_unique_id)")
        return buf.raw

    def rccl_init(self, uid, rank, world):
        self._ck(self._L.bce_rccl_init(self.h, bytes(uid), int(rank), int(world)))

    def rccl_comm_info(self):
        """(ranks RCCL sees, this rank, HIP device) of the context's communicator"""
        out = (C.c_int * 3)()
        self._ck(self._L.bce_rccl_comm_info(self.h, out))
        return {"ranks": int(out[0]), "rank": int(out[1]), "device": int(out[2])}

    def rccl_shutdown(self):
        self._ck(self._L.bce_rccl_shutdown(self.h))

    def rccl_allgather(self, dev_send_ptr, dev_recv_ptr, nbytes):
        self._ck(self._L.bce_rccl_allgather(self.h, C.c_void_p(dev_send_ptr), C.c_void_p(dev_recv_ptr), int(nbytes)))

    def bytes_per_bootstrap_parts(self):
        buf = (C.c_uint64 * 3)()
        self._ck(self._L.bce_bytes_per_bootstrap_parts(self.h, buf))
        return {"bsk": int(buf[0]), "ksk": int(buf[1]), "ct": int(buf[2])}

    def is64(self):
        """ring modulus >= 2^28: the 64-bit kernels (kernels64.hip)"""
        return self.params["Q"] >= (1 << 28)

    def fp64(self):
        """64-bit path computing with exact integers in IEEE doubles (Q < 2^39, unless BCE_FP64=0)"""
        return self.is64() and self.params["Q"] < (1 << 39) and os.environ.get("BCE_FP64", "1")[:1] != "0"

    def bsk_word_bytes(self):
        return 8 if self.is64() else 4

    def forward_transforms_per_step(self):
        return int(self._L.bce_forward_transforms_per_step(self.h))

    def forward_units(self):
        """1: saturated launches transform as 24 quarter units, three per wave; 0: whole-row + half-row bodies"""
        return int(self._L.bce_forward_units(self.h))

    def forward_mfma(self):
        """1: the quarter units run the stages on bits 9..4 as i8 matrix products (BCE_FWD_MFMA=0: the quarter-unit body)"""
        return int(self._L.bce_forward_mfma(self.h))

    def lazy_arithmetic(self):
        """1: the 32-bit kernels run their lazy forms (the bounds of derive_ctx hold for this Q); 0: the corrected forms"""
        return int(self._L.bce_lazy_arithmetic(self.h))

    def launch_capacity(self):
        lone, full = C.c_uint32(), C.c_uint32()
        self._ck(self._L.bce_launch_capacity(self.h, C.byref(lone), C.byref(full)))
        return int(lone.value), int(full.value)

    # --- staged outputs for parity ---
    def debug_eval_stages(self, descs):
        """(acc, lweN, ks) of one frontier; with pair descriptors (PAIR) lweN and ks carry one more row per pair, in
        descriptor order, after the len(descs) rows of the first outputs"""
        arr = make_descs(descs)
        nb = len(arr)
        rows = nb + sum(1 for d in arr if (d.op >> 8) & 0xFF)
        acc = np.zeros((nb, 2 * self.N), dtype=np.uint64)
        lweN = np.zeros((rows, self.N + 1), dtype=np.uint64)
        ks = np.zeros((rows, self.n + 1), dtype=np.uint64)
        self._ck(self._L.bce_debug_eval_stages(self.h, nb, arr, _p(acc), _p(lweN), _p(ks)))
        return acc, lweN, ks

    def debug_tail(self, acc, out_slots):
        """the tail of EvalBinGate alone on caller-supplied coefficient-form accumulators [count][2][N];
        refreshed ciphertexts go to out_slots; returns (lweN mod qKS, ks mod qKS)"""
        acc = np.ascontiguousarray(acc, dtype=np.uint64).reshape(-1, 2 * self.N)
        slots = np.ascontiguousarray(out_slots, dtype=np.uint32)
        assert slots.size == acc.shape[0]
        lweN = np.zeros((slots.size, self.N + 1), dtype=np.uint64)
        ks = np.zeros((slots.size, self.n + 1), dtype=np.uint64)
        self._ck(self._L.bce_debug_tail(self.h, slots.size, _p(acc), _p(slots), _p(lweN), _p(ks)))
        return lweN, ks

    def debug_tail_split(self, count):
        """workgroups the separate tail kernels spread one bootstrap over in a launch of `count` bootstraps (launch_tail's rule)"""
        return int(self._L.bce_debug_tail_split(self.h, int(count)))

    def debug_ntt(self, polys, inverse=False):
        polys = np.array(polys, dtype=np.uint64, order="C")
        count = polys.size // self.N
        self._ck(self._L.bce_debug_ntt(self.h, _p(polys), count, 1 if inverse else 0))
        return polys


# =====================================================================================
# host circuit runtime (include/bce_circuit.h)
# =====================================================================================
class CircuitInfo(C.Structure):
    _fields_ = [("n_gates", C.c_uint32), ("n_input_gates", C.c_uint32), ("n_wires", C.c_uint32),
                ("n_inputs", C.c_uint32), ("n_input_bits", C.c_uint32 * 2), ("n_output_bits", C.c_uint32),
                ("n_levels", C.c_uint32), ("n_sublaunches", C.c_uint32), ("n_relevel_steps", C.c_uint32),
                ("max_frontier", C.c_uint32), ("slot_stride", C.c_uint32),
                ("n_bootstraps", C.c_uint64)]


class CircuitStats(C.Structure):
    _fields_ = [("total_ms", C.c_double), ("management_ms", C.c_double), ("execution_ms", C.c_double),
                ("bootstraps", C.c_uint64), ("levels", C.c_uint32), ("sublaunches", C.c_uint32),
                ("verify_fixes", C.c_uint32), ("exchanges", C.c_uint32), ("exchanged_cts", C.c_uint64)]


ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_int)

CIRCUIT_SYMBOLS = [
    "bce_circuit_create", "bce_circuit_destroy", "bce_circuit_last_error", "bce_circuit_read_file",
    "bce_circuit_read_bristol", "bce_circuit_get_info", "bce_circuit_reset", "bce_circuit_rearm", "bce_circuit_set_plaintext",
    "bce_circuit_set_encrypted", "bce_circuit_set_verify", "bce_circuit_get_flags", "bce_circuit_set_batched",
    "bce_circuit_set_encrypt_mode", "bce_circuit_get_encrypt_mode", "bce_circuit_plan_hash", "bce_circuit_set_shard_locality", "bce_circuit_set_xor_fast", "bce_circuit_set_xor_shared", "bce_circuit_xor_shared_active", "bce_circuit_set_xor_single", "bce_circuit_get_xor_single", "bce_circuit_set_relevel", "bce_circuit_get_relevel", "bce_circuit_set_dataflow", "bce_circuit_set_dataflow_shared", "bce_circuit_dataflow_active", "bce_circuit_set_graph", "bce_circuit_graph_active", "bce_circuit_set_device_verify", "bce_circuit_device_verify_active", "bce_circuit_get_check_report", "bce_circuit_resolve_mode", "bce_circuit_dataflow_plan", "bce_circuit_set_balance", "bce_circuit_relevel_steps", "bce_circuit_relevel_descs", "bce_circuit_relevel_publications", "bce_circuit_check_relevel", "bce_circuit_set_instances", "bce_circuit_set_input", "bce_circuit_clock",
    "bce_circuit_set_instance_keysets", "bce_circuit_get_output", "bce_circuit_get_buses", "bce_circuit_get_counts", "bce_circuit_get_stats", "bce_circuit_dump",
    "bce_circuit_set_exchange", "bce_circuit_enable_rccl", "bce_circuit_exchange_capacity", "bce_assemble_bristol", "bce_pool_gather",
    "bce_pool_scatter",
]

_circ_bound = False


def _bind_circuit():
    global _circ_bound
    L = lib()
    if _circ_bound:
        return L
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
    L.bce_circuit_create.argtypes = [vp, C.POINTER(vp)]
    L.bce_circuit_destroy.argtypes = [vp]
    L.bce_circuit_destroy.restype = None
    L.bce_circuit_last_error.argtypes = [vp]
    L.bce_circuit_last_error.restype = C.c_char_p
    L.bce_circuit_read_file.argtypes = [vp, C.c_char_p]
    L.bce_circuit_read_bristol.argtypes = [vp, C.c_char_p, i32]
    L.bce_circuit_get_info.argtypes = [vp, C.POINTER(CircuitInfo)]
    for name in ("reset", "rearm", "clock"):
        getattr(L, "bce_circuit_" + name).argtypes = [vp]
    for name in ("set_plaintext", "set_encrypted", "set_verify", "set_batched", "set_encrypt_mode", "set_xor_fast", "set_xor_shared", "set_xor_single", "set_relevel", "dump"):
        getattr(L, "bce_circuit_" + name).argtypes = [vp, i32]
    L.bce_circuit_get_flags.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.bce_circuit_set_instances.argtypes = [vp, u32]
    L.bce_circuit_set_instance_keysets.argtypes = [vp, vp, u32]
    L.bce_circuit_set_balance.argtypes = [vp, i32, u32, u32]
    L.bce_circuit_set_dataflow.argtypes = [vp, i32]
    L.bce_circuit_set_dataflow_shared.argtypes = [vp, i32]
    L.bce_circuit_set_graph.argtypes = [vp, i32]
    L.bce_circuit_graph_active.argtypes = [vp]
    L.bce_circuit_set_device_verify.argtypes = [vp, i32]
    L.bce_circuit_device_verify_active.argtypes = [vp]
    L.bce_circuit_get_check_report.argtypes = [vp, C.POINTER(CheckReport)]
    L.bce_circuit_resolve_mode.argtypes = [u32]
    L.bce_circuit_resolve_mode.restype = u32
    L.bce_circuit_get_encrypt_mode.argtypes = [vp]
    L.bce_circuit_get_relevel.argtypes = [vp]
    L.bce_circuit_set_shard_locality.argtypes = [vp, i32]
    L.bce_circuit_plan_hash.argtypes = [vp]
    L.bce_circuit_plan_hash.restype = u64
    L.bce_circuit_dataflow_active.argtypes = [vp]
    L.bce_circuit_xor_shared_active.argtypes = [vp]
    L.bce_circuit_get_xor_single.argtypes = [vp]
    L.bce_circuit_dataflow_plan.argtypes = [vp, vp, vp, u32, C.POINTER(u32)]
    L.bce_circuit_relevel_steps.argtypes = [vp, C.POINTER(u32), u32, C.POINTER(u32)]
    L.bce_circuit_relevel_descs.argtypes = [vp, vp, u32, C.POINTER(u32)]
    L.bce_circuit_relevel_publications.argtypes = [vp, C.POINTER(u32), u32, C.POINTER(u32)]
    L.bce_circuit_check_relevel.argtypes = [vp]
    L.bce_circuit_set_input.argtypes = [vp, u32, vp, u32, vp]
    L.bce_circuit_get_output.argtypes = [vp, u32, vp]
    L.bce_circuit_get_buses.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), u32, C.POINTER(u32), C.POINTER(u32), u32]
    L.bce_circuit_get_counts.argtypes = [vp, C.POINTER(u32 * 6)]
    L.bce_circuit_get_stats.argtypes = [vp, C.POINTER(CircuitStats)]
    L.bce_circuit_set_exchange.argtypes = [vp, u32, u32, i32, ALLGATHER_FN, vp, vp, vp, vp, vp, u64]
    L.bce_circuit_enable_rccl.argtypes = [vp, i32]
    L.bce_circuit_exchange_capacity.argtypes = [vp, u32, i32, i32]
    L.bce_circuit_exchange_capacity.restype = u64
    L.bce_assemble_bristol.argtypes = [C.c_char_p, i32, i32, i32, C.c_char_p, C.c_char_p, u32]
    L.bce_pool_gather.argtypes = [vp, vp, u32, vp]
    L.bce_pool_scatter.argtypes = [vp, vp, u32, vp]
    _circ_bound = True
    return L


def assemble_bristol(in_path, out_path=None, new_flag=False, gen_fan_flag=False, debug_flag=False):
    """analyze_bristol + assemble_bristol (src/analyze.cpp:56, src/assemble.cpp:46)."""
    L = _bind_circuit()
    err = C.create_string_buffer(512)
    rc = L.bce_assemble_bristol(in_path.encode(), int(new_flag), int(gen_fan_flag), int(debug_flag),
                                out_path.encode() if out_path else None, err, 512)
    if rc != OK:
        raise BceError(rc, err.value.decode())


def circuit_resolve_mode(inputs):
    """the rule that decides what a Clock() runs, as bits (bce_circuit_resolve_mode of bce_circuit.h); no circuit, no GPU"""
    return int(_bind_circuit().bce_circuit_resolve_mode(int(inputs)))


# bit-order helpers of the reference harnesses (src/utils.cpp:49-89)
def HexStr2UintVec(inhex):
    """element 0 = LSB of the whole number: walk the string from its last character, nibble LSB-first"""
    out = []
    for ch in reversed(inhex):
        v = int(ch, 16)
        out.extend([(v >> b) & 1 for b in range(4)])
    return out


def BinStr2UintVec(inbin):
    """element 0 = last character"""
    return [int(ch) for ch in reversed(inbin)]


class Circuit:
    """Mirror of the reference's Circuit driver API (src/circuit.h:54-73)."""

    def __init__(self, cc=None):
        self._L = _bind_circuit()
        self.cc = cc
        h = C.c_void_p()
        rc = self._L.bce_circuit_create(cc.h if cc is not None else None, C.byref(h))
        if rc != OK:
            raise BceError(rc, "bce_circuit_create failed")
        self.h = h
        self._keep = []

    def _ck(self, rc):
        if rc != OK:
            raise BceError(rc, self._L.bce_circuit_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self._L.bce_circuit_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def ReadFile(self, path):
        self._ck(self._L.bce_circuit_read_file(self.h, path.encode()))
        return True

    def ReadBristol(self, path, new_flag=False):
        self._ck(self._L.bce_circuit_read_bristol(self.h, path.encode(), int(new_flag)))
        return True

    def info(self):
        i = CircuitInfo()
        self._ck(self._L.bce_circuit_get_info(self.h, C.byref(i)))
        d = {k: getattr(i, k) for k, _ in CircuitInfo._fields_ if k != "n_input_bits"}
        ins, outs = self.buses()
        d["n_input_bits"] = ins + [0] * (2 - len(ins))    # at least two entries, as the reference's two-input header
        d["output_buses"] = outs
        return d

    def buses(self):
        """(input bus widths, output bus widths) -- Bristol Fashion headers may name any number of either"""
        ni, no = C.c_uint32(), C.c_uint32()
        iw, ow = (C.c_uint32 * 64)(), (C.c_uint32 * 64)()
        self._ck(self._L.bce_circuit_get_buses(self.h, C.byref(ni), iw, 64, C.byref(no), ow, 64))
        ins = [int(iw[k]) for k in range(min(64, ni.value))]
        while len(ins) > 1 and ins[-1] == 0:
            ins.pop()
        return ins, [int(ow[k]) for k in range(min(64, no.value))]

    def Reset(self):
        self._ck(self._L.bce_circuit_reset(self.h))

    def Rearm(self):
        self._ck(self._L.bce_circuit_rearm(self.h))

    def setPlaintext(self, b):
        self._ck(self._L.bce_circuit_set_plaintext(self.h, int(b)))

    def setEncrypted(self, b):
        self._ck(self._L.bce_circuit_set_encrypted(self.h, int(b)))

    def setVerify(self, b):
        self._ck(self._L.bce_circuit_set_verify(self.h, int(b)))

    def _flags(self):
        p, e, v = C.c_int(), C.c_int(), C.c_int()
        self._ck(self._L.bce_circuit_get_flags(self.h, C.byref(p), C.byref(e), C.byref(v)))
        return bool(p.value), bool(e.value), bool(v.value)

    def getPlaintext(self):
        return self._flags()[0]

    def getEncrypted(self):
        return self._flags()[1]

    def getVerify(self):
        return self._flags()[2]

    def setBatched(self, b):
        self._ck(self._L.bce_circuit_set_batched(self.h, int(b)))

    def setEncryptMode(self, mode):
        """BOOTSTRAPPED (default, OpenFHE v1.0.x's cc.Encrypt) or FRESH"""
        self._ck(self._L.bce_circuit_set_encrypt_mode(self.h, int(mode)))

    def setShardLocality(self, on):
        """gate sharding: units follow their inputs' ranks (default) / contiguous split in netlist order"""
        self._ck(self._L.bce_circuit_set_shard_locality(self.h, int(on)))

    def plan_hash(self):
        """digest of the sharding plan: must be equal on every rank of a run"""
        return int(self._L.bce_circuit_plan_hash(self.h))

    def getEncryptMode(self):
        return int(self._L.bce_circuit_get_encrypt_mode(self.h))

    def setXorFast(self, b):
        """opt-in, not reference semantics: XOR as one XOR_FAST bootstrap"""
        self._ck(self._L.bce_circuit_set_xor_fast(self.h, int(b)))

    def setXorShared(self, b):
        """opt-in: XOR as AND(OR, NAND) with the OR and the NAND from one blind rotation (a PAIR descriptor): two blind
        rotations per XOR instead of three, same depth, same bits on every netlist wire; before SetInput, not with setXorFast"""
        self._ck(self._L.bce_circuit_set_xor_shared(self.h, int(b)))

    def setXorSingle(self, b):
        """opt-in, not an OpenFHE gate: XOR as one XOR bootstrap (op XOR) of ct1 + ct2 with a three-level test polynomial: the
        count and depth of XOR_FAST at a plain gate's noise; before SetInput, not with setXorFast / setXorShared"""
        self._ck(self._L.bce_circuit_set_xor_single(self.h, int(b)))

    def getXorSingle(self):
        return bool(self._L.bce_circuit_get_xor_single(self.h))

    def xorSharedActive(self):
        """True if the next Clock() on the bootstrap-depth schedule lowers its XORs that way (batched launches, no gate
        sharding, no host-side verify pass)"""
        return bool(self._L.bce_circuit_xor_shared_active(self.h))

    def setRelevel(self, b):
        """bootstrap-depth schedule (fewer dependent launches, same ciphertexts): the default; False = the reference's
        gate-level Clock rounds (src/circuit.cpp:532-573)"""
        self._ck(self._L.bce_circuit_set_relevel(self.h, int(b)))

    def getRelevel(self):
        return bool(self._L.bce_circuit_get_relevel(self.h))

    def setDataflow(self, b):
        """opt-in: the whole bootstrap DAG in one persistent launch (device-side ready-gate rule); before SetInput"""
        self._ck(self._L.bce_circuit_set_dataflow(self.h, int(b)))

    def setDataflowShared(self, b):
        """opt-in on top of setDataflow and setXorShared: the shared XORs stay on the dataflow schedule as pair tasks
        (dataflowActive() and xorSharedActive() both True); without it the two together run the step schedule; before SetInput"""
        self._ck(self._L.bce_circuit_set_dataflow_shared(self.h, int(b)))

    def dataflow_plan(self):
        """(tasks, priority classes) of the dataflow schedule: tasks = (op, in0, in1, out, neg0, neg1), one instance"""
        n = C.c_uint32(0)
        self._ck(self._L.bce_circuit_dataflow_plan(self.h, None, None, 0, C.byref(n)))
        arr = (GateDesc * max(1, n.value))()
        pr = (C.c_uint8 * max(1, n.value))()
        self._ck(self._L.bce_circuit_dataflow_plan(self.h, arr, pr, n.value, C.byref(n)))
        return ([(a.op, a.in0, a.in1, a.out, a.neg0, a.neg1) for a in arr[:n.value]], [int(x) for x in pr[:n.value]])

    def setGraph(self, b):
        """replay the bootstrap-depth schedule as one hipGraph per Clock() (bce_plan_run); opt-in, same ciphertexts"""
        self._ck(self._L.bce_circuit_set_graph(self.h, int(b)))

    def graphActive(self):
        return bool(self._L.bce_circuit_graph_active(self.h))

    def setDeviceVerify(self, b):
        """opt-in: verify mode's decrypt / compare / repair on the device, between the steps of the bootstrap-depth schedule
        (src/gate.cpp:153-160); a repaired register holds the trivial ciphertext of the right bit.  With setDataflow the
        same checks run inside the persistent kernel, before a finished bootstrap releases its consumers"""
        self._ck(self._L.bce_circuit_set_device_verify(self.h, int(b)))

    def deviceVerifyActive(self):
        return bool(self._L.bce_circuit_device_verify_active(self.h))

    def check_report(self):
        """the device's report of the last Clock() in device verify mode, with noise_rms = sqrt(sum_sq_err / checked) and
        margin = q/8 - max_abs_err"""
        r = CheckReport()
        self._ck(self._L.bce_circuit_get_check_report(self.h, C.byref(r)))
        return _report_dict(r, self.cc.params["q"] if self.cc is not None else 0)

    def dataflowActive(self):
        return bool(self._L.bce_circuit_dataflow_active(self.h))

    def setInstances(self, k):
        self._ck(self._L.bce_circuit_set_instances(self.h, int(k)))

    def setInstanceKeys(self, keysets):
        """instance k is encrypted, evaluated and decrypted under key set keysets[k] of the engine (one id per instance, before
        SetInput; an empty list returns to the selected set).  Not with setDataflow, setVerify, setDeviceVerify or gate sharding."""
        ids = np.ascontiguousarray(keysets, dtype=np.uint32)
        self._ck(self._L.bce_circuit_set_instance_keysets(self.h, _p(ids) if ids.size else None, ids.size))

    def setBalance(self, on, lone=0, full=0):
        """bootstrap-depth schedule filled by slack up to the engine's launch staircase (default on); before SetInput"""
        self._ck(self._L.bce_circuit_set_balance(self.h, int(on), int(lone), int(full)))

    def relevel_steps(self):
        """bootstraps per step of the bootstrap-depth schedule, one instance"""
        n = C.c_uint32(0)
        self._ck(self._L.bce_circuit_relevel_steps(self.h, None, 0, C.byref(n)))
        buf = (C.c_uint32 * max(1, n.value))()
        self._ck(self._L.bce_circuit_relevel_steps(self.h, buf, n.value, C.byref(n)))
        return [int(buf[i]) for i in range(n.value)]

    def relevel_plan(self):
        """test and debug API: the bootstrap-depth schedule's descriptors, one list of (op, in0, in1, out, neg0, neg1) per
        step, slots of instance 0, for replaying a schedule descriptor by descriptor on the oracle"""
        n = C.c_uint32(0)
        self._ck(self._L.bce_circuit_relevel_descs(self.h, None, 0, C.byref(n)))
        buf = (GateDesc * max(1, n.value))()
        self._ck(self._L.bce_circuit_relevel_descs(self.h, buf, n.value, C.byref(n)))
        flat = [(d.op, d.in0, d.in1, d.out, d.neg0, d.neg1) for d in buf[:n.value]]
        steps, at = [], 0
        for size in self.relevel_steps():
            steps.append(flat[at:at + size])
            at += size
        return steps

    def relevel_publications(self):
        """registers this rank publishes after each step of the bootstrap-depth schedule (gate sharding)"""
        n = C.c_uint32(0)
        self._ck(self._L.bce_circuit_relevel_publications(self.h, None, 0, C.byref(n)))
        buf = (C.c_uint32 * max(1, n.value))()
        self._ck(self._L.bce_circuit_relevel_publications(self.h, buf, n.value, C.byref(n)))
        return [int(buf[i]) for i in range(n.value)]

    def check_relevel(self):
        self._ck(self._L.bce_circuit_check_relevel(self.h))

    def SetInput(self, inputs, instance=0):
        """inputs[k][bit], LSB = index 0 (the reference's Inputs type)"""
        widths = np.array([len(b) for b in inputs], dtype=np.uint32)
        bits = np.array([v for b in inputs for v in b], dtype=np.uint8)
        if bits.size == 0:
            bits = np.zeros(1, dtype=np.uint8)
        self._ck(self._L.bce_circuit_set_input(self.h, int(instance), _p(widths), len(inputs), _p(bits)))

    def Clock(self, instance=0):
        self._ck(self._L.bce_circuit_clock(self.h))
        return self.Outputs(instance)

    def Outputs(self, instance=0):
        """Outputs[k][bit] like the reference (one list per output value; the reference's circuits have one)"""
        i = CircuitInfo()
        self._ck(self._L.bce_circuit_get_info(self.h, C.byref(i)))
        n = i.n_output_bits
        out = np.zeros(max(n, 1), dtype=np.uint8)
        self._ck(self._L.bce_circuit_get_output(self.h, int(instance), _p(out)))
        bits = [int(v) for v in out[:n]]
        widths = self.buses()[1] or [n]
        res, pos = [], 0
        for w in widths:
            res.append(bits[pos:pos + w])
            pos += w
        return res

    def counts(self):
        c = (C.c_uint32 * 6)()
        self._ck(self._L.bce_circuit_get_counts(self.h, C.byref(c)))
        return dict(zip(["input", "output", "not", "and", "or", "xor"], [int(v) for v in c]))

    def stats(self):
        s = CircuitStats()
        self._ck(self._L.bce_circuit_get_stats(self.h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in CircuitStats._fields_}

    def dumpGateCount(self):
        self._ck(self._L.bce_circuit_dump(self.h, 2))

    def enable_rccl(self, on=True):
        """device payloads of the exchange through the in-library RCCL all-gather (after cc.rccl_init)"""
        self._ck(self._L.bce_circuit_enable_rccl(self.h, int(on)))

    def exchange_capacity(self, world, shard_mode, encrypted):
        return int(self._L.bce_circuit_exchange_capacity(self.h, world, shard_mode, int(encrypted)))

    def set_exchange(self, rank, world, shard_mode, fn, host_send, host_recv, dev_send, dev_recv, capacity):
        """fn(bytes, on_device) -> 0 on success; buffers are raw addresses (e.g. tensor.data_ptr())"""
        cb = ALLGATHER_FN(lambda user, nbytes, on_dev: int(fn(int(nbytes), int(on_dev))))
        self._keep.append(cb)
        self._ck(self._L.bce_circuit_set_exchange(self.h, rank, world, shard_mode, cb, None, host_send, host_recv,
                                                  dev_send, dev_recv, capacity))
