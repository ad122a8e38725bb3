/*
 * bce_gpu.h -- C ABI of the MI355X gate-bootstrapping engine (libbce_amd.so).
 *
 * This is the drop-in boundary for the ONE hot path of
 * openfheorg/openfhe-boolean-circuit-evaluator: everything the reference
 * reaches through `lbcrypto::BinFHEContext` (OpenFHE).  Each entry point cites
 * the reference interface it replaces (paths relative to the reference root).
 * Plain C types only; no exception crosses this boundary: every call returns a
 * bce_status and bce_last_error() holds the message.
 *
 * The per-gate call `cc.EvalBinGate(gate, ct1, ct2)` made inside one OpenMP
 * task per gate (src/circuit.cpp:698-710 -> src/gate.cpp:133,172,200-202)
 * becomes ONE call bce_eval_gates() for the whole ready-gate frontier; LWE
 * ciphertexts live in a device-resident pool and are named by slot index
 * (the reference's `CipherText` alias, src/wire.h:46).
 */
#ifndef BCE_GPU_H
#define BCE_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bce_ctx bce_ctx;

/* lbcrypto::BINFHE_PARAMSET as used at src/utils.cpp:167-172, src/circuit.cpp:69-78
 * (the reference accepts TOY and STD128_OPT; the rest are OpenFHE's table rows). */
enum bce_paramset {
    BCE_TOY = 0, BCE_MEDIUM = 1, BCE_STD128_AP = 2, BCE_STD128_APOPT = 3, BCE_STD128 = 4,
    BCE_STD128_OPT = 5, BCE_STD192 = 6, BCE_STD192_OPT = 7, BCE_STD256 = 8, BCE_STD256_OPT = 9
};
/* lbcrypto::BINFHE_METHOD, src/utils.cpp:180-185 */
enum bce_method { BCE_AP = 1, BCE_GINX = 2 };
/* lbcrypto::BINGATE for EvalBinGate (src/gate.cpp:133,172) + the unary ops the driver issues */
enum bce_op {
    BCE_OR = 0, BCE_AND = 1, BCE_NOR = 2, BCE_NAND = 3, BCE_XOR_FAST = 4, BCE_XNOR_FAST = 5,
    BCE_XOR = 0x10006,   /* XOR in one bootstrap of ct1 + ct2: three-level test polynomial, see below; NOT an OpenFHE gate.
                            Gate byte 6 with bit 16 set: the bare codes 6 .. 15 and 19 .. 255 stay no op (BCE_ERR_ARG), as they always were */
    BCE_OP_NOT = 16,     /* EvalNOT, src/gate.cpp:112,198-199 : no bootstrap      */
    BCE_OP_REFRESH = 17, /* Bootstrap(ct) as run by Encrypt(BOOTSTRAPPED)         */
    BCE_OP_COPY = 18     /* OUTPUT gate copy, src/gate.cpp:90-94                  */
};
enum bce_status {
    BCE_OK = 0, BCE_ERR_ARG = 1, BCE_ERR_NO_DEVICE = 2, BCE_ERR_HIP = 3, BCE_ERR_NO_KEYS = 4,
    BCE_ERR_POOL = 5, BCE_ERR_UNSUPPORTED = 6, BCE_ERR_STATE = 7
};
/* lbcrypto::BINFHE_OUTPUT of BinFHEContext::Encrypt (v1.0.x default is BOOTSTRAPPED) */
enum bce_encrypt_mode { BCE_FRESH = 0, BCE_BOOTSTRAPPED = 1 };

/* parameter block (all u64), same order as the oracle's */
enum { BCE_P_n = 0, BCE_P_N, BCE_P_q, BCE_P_Q, BCE_P_qKS, BCE_P_baseKS, BCE_P_dKS, BCE_P_baseG, BCE_P_dG,
       BCE_P_baseR, BCE_P_dR, BCE_P_method, BCE_P_psi, BCE_P_COUNT };

/* One gate of the frontier.  `neg0/neg1` fold EvalNOT of an input into the
 * bootstrap's LWE prep, which is how XOR = (a AND !b) OR (!a AND b)
 * (src/gate.cpp:198-202) is issued without materialising the NOTs. */
typedef struct bce_gate_desc {
    uint32_t op;   /* enum bce_op: the gate in bits 0..7; bits 8..15: 0, or the second gate + 1 of a pair (BCE_PAIR); bit 16: BCE_XOR only */
    uint32_t in0;  /* pool slot */
    uint32_t in1;  /* pool slot (ignored by 1-input ops) */
    uint32_t out;  /* pool slot */
    uint32_t neg0;
    uint32_t neg1;
} bce_gate_desc;

/* Two gates from ONE blind rotation.  The four plain gates differ only in the window constant q1 of BootstrapGateCore's
 * test polynomial m, which depends on b and q1 through (b - q1) mod q alone, so m_{q1'} = X^e m_{q1} (mod X^N + 1) with
 * e = ((q1 - q1') mod q) (2N / q); the monomial commutes with the blind rotation.  A pair descriptor runs the blind rotation
 * of `op` once and the tail (extract, ModSwitch, KeySwitch, ModSwitch) twice, on acc and on X^e acc:
 *   slot out     <- op (in0', in1')      (word for word what the plain descriptor writes)
 *   slot out + 1 <- op2(in0', in1')      (out + 1 + k * slot_stride with instances)
 * with the same neg0 / neg1 for both.  The second output decrypts like EvalBinGate(op2, ...) but is NOT word-identical to
 * it (the gadget decomposition's rounding is not symmetric under the rotation); its noise is that of a plain gate.
 * Legal: op and op2 two DIFFERENT gates of BCE_OR, BCE_AND, BCE_NOR, BCE_NAND; anything else in bits 8.. is BCE_ERR_ARG.
 * out + 1 obeys every rule out obeys (pool bound: BCE_ERR_POOL; written by this call, read by none of it).
 * Accepted by bce_eval_gates, bce_eval_gates_strided, bce_plan_create, bce_debug_eval_stages and bce_dag_create_pairs;
 * bce_dag_create refuses pairs (BCE_ERR_UNSUPPORTED).  The counters of bce_timing count blind rotations: a pair counts 1.
 * XOR(a, b) = AND(OR(a, b), NAND(a, b)) is then two blind rotations instead of three (bce_circuit_set_xor_shared). */
#define BCE_PAIR(op, op2) ((uint32_t)(op) | (((uint32_t)(op2) + 1u) << 8))

/* XOR in ONE bootstrap at a plain gate's noise (BCE_XOR; NOT a gate of OpenFHE v1.0.x, whose one-bootstrap XOR is XOR_FAST).
 * The plain sum ct1 + ct2 of two bits encoded in multiples of q/4 (with the folded EvalNOTs of neg0 / neg1, exactly the
 * preparation of AND and OR) has phase 0, q/4 or q/2, and XOR is 1 exactly at q/4.  With f = 2N/q, b the last word of the sum
 * and one = 2(Q/8 + 1) mod Q the test polynomial is, for j = 0 .. q/2 - 1 and t = (b - j) mod q,
 *   m[j f] = one       if  q/8 <= t < 3q/8
 *   m[j f] = Q - one   if 5q/8 <= t < 7q/8
 *   m[j f] = 0         otherwise                     (every other coefficient 0)
 * i.e. the function +one on [q/8, 3q/8), -one on [5q/8, 7q/8), 0 elsewhere, which is negacyclic (f(t + q/2) = -f(t)) and so a
 * legal test polynomial of the same blind rotation; the tail extracts b' = acc[1][0] WITHOUT the Q/8 + 1 every other gate adds,
 * so the nominal outputs are 0 and 2(Q/8 + 1), the levels of every other gate: consumers need no change.
 * Margin: each level (0, q/4, q/2) is q/8 away from BOTH neighbouring boundaries, where a plain gate has q/8 on its near side;
 * the input noise is that of AND's sum (XOR_FAST doubles it: 2(ct1 - ct2) in OR's window), so the failure probability is at
 * most twice a plain gate's one-sided tail.  Output noise is a plain gate's: the accumulator's noise comes from the external
 * products, not from the polynomial's values.  neg0 / neg1 negate the inputs; XNOR is BCE_XOR with one of them set.
 * Accepted wherever a plain gate is (bce_eval_gates[_strided], bce_debug_eval_stages, bce_plan_create, bce_dag_create[_pairs]),
 * one bootstrap in bce_timing; NOT inside BCE_PAIR (its polynomial is no rotation of a plain gate's): BCE_ERR_ARG.
 * The word is 0x10006 and nothing else: the code 6 alone, and bit 16 on any other word, are BCE_ERR_ARG.
 * bce_circuit_set_xor_single evaluates every XOR gate of a circuit this way. */

/* which blind-rotation kernel a launch used (chosen by parameter set and launch size) */
enum bce_br_kernel {
    BCE_BR_WAVE_PER_TRANSFORM = 0, /* k_blind_rotate: one wave per (inverse) transform, up to 3 workgroups / CU */
    BCE_BR_SPLIT_X1 = 1,           /* k_blind_rotate_lat<LatVariant<2, ...>>: split inverse transform, launches of <= #CU workgroups */
    BCE_BR_SPLIT_X2 = 2,           /* k_blind_rotate_lat<LatVariant<4, ...>>: same, register budget for two workgroups per CU */
    BCE_BR_WORD64 = 3,             /* ring modulus >= 2^28: the integer 64-bit and fp64 families of kernel_class() (csrc/kernels.hpp),
                                      reported by launch_blind_rotate like the other three */
    BCE_BR_DAG = 4,                /* k_bootstrap_dag: one persistent launch per bce_dag_run (tail fused) */
    BCE_BR_GRAPH = 5,              /* bce_plan_run: the launches of a whole step schedule replayed as one hipGraph (timed as one) */
    BCE_BR_KERNELS = 6
};

/* cumulative device timing, measured with HIP events on the engine's stream */
typedef struct bce_timing {
    double   blind_rotate_ms;   /* sum over launches of the blind-rotation kernels */
    double   tail_ms;           /* extract + modswitch + keyswitch + modswitch    */
    uint64_t blind_rotate_launches;
    uint64_t bootstraps;        /* blind rotations executed (NOT/COPY not counted; a BCE_PAIR descriptor counts 1) */
    /* the same three blind-rotation figures per kernel (index: enum bce_br_kernel) */
    double   br_ms[BCE_BR_KERNELS];
    uint64_t br_launches[BCE_BR_KERNELS];
    uint64_t br_bootstraps[BCE_BR_KERNELS];
    uint64_t fused_tail_launches; /* launches whose blind-rotation kernel also ran the tail in its epilogue
                                     (their tail time is inside blind_rotate_ms, not tail_ms) */
} bce_timing;

/* ---- context ----------------------------------------------------------- */
/* BinFHEContext() + GenerateBinFHEContext(set, method): src/circuit.cpp:65,88.
 * device = HIP device ordinal.  Fails with BCE_ERR_NO_DEVICE when no GPU is
 * visible: there is no CPU fallback in the product. */
int bce_ctx_create(int paramset, int method, int device, bce_ctx** out);
int bce_ctx_create_custom(uint32_t n, uint32_t N, uint64_t q, uint64_t Q, uint64_t qKS, uint32_t baseKS,
                          uint32_t baseG, uint32_t baseR, int method, int device, bce_ctx** out);
void bce_ctx_destroy(bce_ctx*);
/* message of the last failing call on this ctx (ctx may be NULL: last create failure) */
const char* bce_last_error(const bce_ctx*);
int bce_get_params(const bce_ctx*, uint64_t out[BCE_P_COUNT]);

/* ---- keys -------------------------------------------------------------- */
/* sk = cc.KeyGen(); cc.BTKeyGen(sk): src/circuit.cpp:90-91.
 * seed == NULL (what a drop-in caller passes): the 32-byte seed comes from the
 * operating system's entropy pool, as OpenFHE's KeyGen draws from its own
 * entropy-seeded PRNG.  An explicit seed makes the keys a deterministic function
 * of it (ChaCha20 streams, DESIGN.md "PRNG spec") -- for the oracle parity tests
 * and for replicating one key set on every rank of a multi-GPU run; whoever passes
 * one owns its secrecy.  RGSW rows are transformed and multiplied by the ring key
 * on the device. */
int bce_keygen(bce_ctx*, const uint8_t seed[32]);
/* canonical exchange format = coefficient domain, u64 words (what an OpenFHE
 * export would be converted to): s[n], z[N] in {-1,0,1}; bsk [i][key][row][col][N]
 * (GINX) or [i][v][k][row][col][N] (AP); ksk [i][v][j][n+1] mod qKS. */
int bce_import_keys(bce_ctx*, const int32_t* s, const int32_t* z, const uint64_t* bsk, uint64_t bsk_words,
                    const uint32_t* ksk, uint64_t ksk_words);
/* Same, with the bootstrapping key already in EVALUATION form as OpenFHE holds it after BTKeyGen: every polynomial in
 * the bit-reversed order of OpenFHE's Cooley-Tukey forward transform (transformnat-impl.h) for psi = the minimal
 * primitive 2N-th root of unity mod Q (bce_get_params: BCE_P_psi; 455622 / 341565 / 13167220 for the tabulated sets) --
 * the engine's own order, so an OpenFHE-side dump needs no SetFormat(COEFFICIENT) pass over the key (12.9 GB for
 * STD192 / AP) and the import needs no transform.  bce_export_bsk_eval is its inverse.
 * PARITY UNPINNED: that this IS OpenFHE's order is recalled, not checked against OpenFHE (absent here) -- it is pinned only
 * against the oracle's own transform.  The gate-vector file of tools/openfhe_export carries NTT records (a polynomial before
 * and after OpenFHE's SetFormat(EVALUATION)) and compare.py checks them with bce_debug_ntt: use this entry point with
 * OpenFHE-made keys only after that check has passed; the coefficient-form import does not depend on the order. */
int bce_import_keys_eval(bce_ctx*, const int32_t* s, const int32_t* z, const uint64_t* bsk_eval, uint64_t bsk_words,
                         const uint32_t* ksk, uint64_t ksk_words);
int bce_export_bsk_eval(bce_ctx*, uint64_t* bsk_eval);
/* The same material from / to a file in the format of tools/openfhe_export/bce_keyfile.h -- what the
 * OpenFHE-side exporter (tools/openfhe_export/export_keys.cpp) writes for the keys of an existing deployment
 * (cc.KeyGen() / cc.BTKeyGen(sk), src/circuit.cpp:90-91).  Parameters in the file must match the context. */
int bce_import_keys_file(bce_ctx*, const char* path);
int bce_export_keys_file(bce_ctx*, const char* path);
uint64_t bce_bsk_words(const bce_ctx*);
uint64_t bce_ksk_words(const bce_ctx*);
int bce_export_sk(const bce_ctx*, int32_t* s, int32_t* z);
int bce_export_bsk(bce_ctx*, uint64_t* bsk);
int bce_export_ksk(bce_ctx*, uint32_t* ksk);

/* ---- key sets ---------------------------------------------------------- */
/* A server evaluates circuits for many clients, each with a bootstrapping and key-switching key of its own.  A context
 * holds up to BCE_MAX_KEYSETS key sets: the secrets, the two evaluation keys and the device copy of the LWE secret of one
 * client.  Everything derived from the parameters alone (tables, kernel choice, pool) stays per context.  Set 0 exists from
 * creation and is what a caller that never touches this section uses.
 *
 * THE RULE: a call that takes no key-set map acts on the set that is SELECTED when it is called.  That covers bce_keygen,
 * the three imports and every export, bce_bsk_words / bce_ksk_words, bce_encrypt_bits (its BOOTSTRAPPED refresh included),
 * bce_decrypt_bits, bce_check_slots, bce_eval_gates[_strided], bce_debug_*, bce_dag_run, and bce_plan_run[_step] of a plan
 * created without a map (a captured plan is captured again when the selection changed).  A selected set without keys gives
 * BCE_ERR_NO_KEYS.
 *
 * bce_keyset_add    creates an empty set; *id = the lowest free id (>= 1).  BCE_ERR_ARG at the limit.
 * bce_keyset_select chooses the selected set (default 0).  BCE_ERR_ARG for an id that does not exist.
 * bce_keyset_drop   synchronises, then frees the set.  BCE_ERR_ARG for set 0, the selected set and an id that does not
 *                   exist; BCE_ERR_STATE while a live plan was created with a map that names the set. */
enum { BCE_MAX_KEYSETS = 256 };
int bce_keyset_add(bce_ctx*, uint32_t* id);
int bce_keyset_select(bce_ctx*, uint32_t id);
int bce_keyset_drop(bce_ctx*, uint32_t id);
uint32_t bce_keyset_count(const bce_ctx*);
uint32_t bce_keyset_selected(const bce_ctx*);

/* ---- device LWE pool --------------------------------------------------- */
/* LWECiphertext objects (src/wire.h:46, src/gate.h:75-78) become slots. */
int bce_pool_reserve(bce_ctx*, uint32_t slots);
uint32_t bce_pool_slots(const bce_ctx*);
/* ciphertext = u64[n+1] (a[0..n), b), the reference's NativeInteger layout */
int bce_lwe_write(bce_ctx*, const uint32_t* slots, uint32_t count, const uint64_t* cts);
int bce_lwe_read(bce_ctx*, const uint32_t* slots, uint32_t count, uint64_t* cts);

/* cc.Encrypt(sk, bit): src/circuit.cpp:506, src/gate.cpp:118,139,143,158,179,211.
 * The mask a and the noise e of every ciphertext come from a ChaCha20 stream keyed
 * with the context's ENCRYPTION seed, which is independent of the key seed: it is
 * drawn from OS entropy when the context is created, and the stream number is a
 * per-context counter that only moves forward -- `enc_index_base` is then IGNORED,
 * so no (a, e) pair can repeat whatever the caller passes (also after
 * bce_import_keys).  BCE_BOOTSTRAPPED also runs Bootstrap(ct) on the device as
 * OpenFHE v1.0.x does by default. */
int bce_encrypt_bits(bce_ctx*, const uint8_t* bits, const uint32_t* slots, uint32_t count,
                     uint64_t enc_index_base, int mode);
/* Test / replication mode of bce_encrypt_bits: with an explicit 32-byte seed,
 * ciphertext k of a call uses stream `enc_index_base + k` of that seed, so that
 * (1) the oracle reproduces the ciphertext bit for bit and (2) every rank of a
 * gate-sharded multi-GPU run encrypts identical inputs.  The caller then owns the
 * uniqueness of the indices: reusing one reuses (a, e).  seed == NULL returns to
 * the default (fresh OS entropy, internal counter). */
int bce_set_encrypt_seed(bce_ctx*, const uint8_t seed[32]);
/* cc.Decrypt(sk, ct, &res): src/circuit.cpp:800, src/gate.cpp:72,97,115,... (res in 0..3) */
int bce_decrypt_bits(bce_ctx*, const uint32_t* slots, uint32_t count, uint8_t* bits);
/* The same with a key-set map per SLOT: slot i is decrypted under set keyset_of_slot[i] ("key sets" above), with the one
 * device gather of the unkeyed call.  Errors as bce_eval_gates_keyed; NULL is bce_decrypt_bits. */
int bce_decrypt_bits_keyed(bce_ctx*, const uint32_t* slots, uint32_t count, const uint32_t* keyset_of_slot /*[count]*/,
                           uint8_t* bits);

/* ---- the hot path ------------------------------------------------------ */
/* Batched EvalBinGate / EvalNOT over one ready frontier:
 * src/circuit.cpp:698-710 + src/gate.cpp:112,133,146,172,198-202.
 * All descriptors of one call are independent (no `out` is an input of the
 * same call).  Asynchronous on the engine's stream; results are ordered with
 * later calls; bce_synchronize() waits. */
int bce_eval_gates(bce_ctx*, uint32_t n_desc, const bce_gate_desc* descs);
/* Same frontier applied to `instances` independent input sets laid out
 * `slot_stride` slots apart (lock-step evaluation of K circuit instances,
 * the reference's sequential numTestLoops loop, src/test_aes.cpp:179-182). */
int bce_eval_gates_strided(bce_ctx*, uint32_t n_desc, const bce_gate_desc* descs, uint32_t instances,
                           uint32_t slot_stride);
/* The same with a key-set map: instance k runs entirely under key set keyset_of_instance[k] (LWE preparation, blind
 * rotation and both tails read that set's keys); several instances may name one set.  One launch, as without a map: the map
 * travels with the descriptors in the same upload.  BCE_ERR_ARG for an id that does not exist, BCE_ERR_NO_KEYS for a named
 * set without keys.  keyset_of_instance == NULL is bce_eval_gates_strided (the selected set). */
int bce_eval_gates_keyed(bce_ctx*, uint32_t n_desc, const bce_gate_desc* descs, uint32_t instances, uint32_t slot_stride,
                         const uint32_t* keyset_of_instance /*[instances]*/);
int bce_synchronize(bce_ctx*);

/* ---- the hot path, a whole step schedule at once ----------------------------------------------------------
 * A circuit's schedule is the same list of frontiers every time it is clocked (src/circuit.cpp:575-683 finds the same
 * ready gates in the same order).  A bce_plan keeps the descriptors of ALL its dependent steps resident on the device:
 *   bce_plan_run_step  = bce_eval_gates_strided for step `s` without the per-call descriptor upload (same kernels,
 *                        same per-launch timing), the caller walks the steps (and may exchange ciphertexts between them);
 *   bce_plan_run       = every step's launches captured once into a hipGraph and replayed with one hipGraphLaunch:
 *                        no per-step host call, no upload, no event between dependent kernels.  Timed as one unit
 *                        (BCE_BR_GRAPH).  Same ciphertexts in every register as the step-by-step form.
 * Steps hold bootstrapped ops only (BCE_OR .. BCE_XNOR_FAST, BCE_XOR, BCE_OP_REFRESH, BCE_PAIR descriptors); `descs` = the steps' descriptors back to
 * back, step s has step_sizes[s] of them.  instances / slot_stride as in bce_eval_gates_strided; the slots are fixed at
 * creation (slot_base shifts them all, e.g. a rank's first instance). */
typedef struct bce_plan bce_plan;
int bce_plan_create(bce_ctx*, uint32_t n_steps, const uint32_t* step_sizes, const bce_gate_desc* descs,
                    uint32_t instances, uint32_t slot_stride, uint32_t slot_base, bce_plan** out);
/* bce_plan_create with a key-set map fixed at creation (copied; resident next to the descriptors): bce_plan_run_step and
 * bce_plan_run (the hipGraph replay) then run instance k under set keyset_of_instance[k], whatever is selected.  Errors as
 * bce_eval_gates_keyed; NULL is bce_plan_create.  bce_plan_set_checks on such a plan: BCE_ERR_UNSUPPORTED. */
int bce_plan_create_keyed(bce_ctx*, uint32_t n_steps, const uint32_t* step_sizes, const bce_gate_desc* descs,
                          uint32_t instances, uint32_t slot_stride, uint32_t slot_base,
                          const uint32_t* keyset_of_instance /*[instances]*/, bce_plan** out);
int bce_plan_run_step(bce_ctx*, bce_plan*, uint32_t step);
int bce_plan_run(bce_ctx*, bce_plan*);
void bce_plan_destroy(bce_ctx*, bce_plan*);

/* ---- verify mode on the device -------------------------------------------------------------------------
 * The reference's harnesses run their encrypted pass with setVerify(true): every gate output is decrypted, compared with
 * the plaintext pass and, on a mismatch, logged ("Bad <OP> fixing") and replaced (src/gate.cpp:113-120,153-160,174-181,
 * 206-213).  The check is one inner product of n words per ciphertext; here it runs on the engine's stream, between the
 * steps of a schedule (or, on the dataflow schedule, inside the persistent kernel: bce_dag_set_checks), against a device
 * copy of the LWE secret (int8, uploaded with the keys):
 *   phase = b - <a, s> mod q;  got = Round(4 phase / q);  err = phase - expect q/4, centred into (-q/2, q/2];
 *   a check is a MISMATCH iff got != expect.
 * Counters accumulate in one report block per context until bce_check_reset; the first BCE_CHECK_LOG_CAP mismatches are
 * also logged (`mismatches` keeps counting beyond that).  err of EVERY checked ciphertext enters max_abs_err / sum_err /
 * sum_sq_err: the measured noise of the run (margin = q/8 - max_abs_err).
 * repair != 0 overwrites a mismatching ciphertext with the TRIVIAL encryption (0, ..., 0, expect q/4).  This deviates from
 * the reference's cc.Encrypt(sk, bit) on purpose: it needs no device PRNG and no host round trip and makes repaired runs
 * bit-reproducible; verify mode holds the secret key and the plaintext anyway, so nothing is disclosed. */
enum { BCE_CHECK_LOG_CAP = 4096 };
typedef struct bce_check_report { uint64_t checked, mismatches, repaired; int64_t sum_err; uint64_t sum_sq_err;
                                  uint32_t max_abs_err, log_count; } bce_check_report;
typedef struct bce_check_entry  { uint32_t tag, index, instance, slot; int32_t err; uint8_t got, expect, pad[2]; } bce_check_entry;
/* Check i of instance k reads slot slots[i] + k * slot_stride against expect[k * count + i] (0..3); the slots of one call
 * are distinct.  Asynchronous, stream-ordered with the gate calls; `tag` comes back in the log entries.
 * BCE_ERR_NO_KEYS without keys, BCE_ERR_POOL for a slot outside the pool, BCE_ERR_ARG for expect > 3 or null pointers. */
int bce_check_slots(bce_ctx*, uint32_t count, const uint32_t* slots, const uint8_t* expect, uint32_t instances,
                    uint32_t slot_stride, int repair, uint32_t tag);
/* Checks attached to a plan: step s checks check_sizes[s] slots (0 allowed), `slots` = the instance-0 numbers of all steps
 * back to back (the plan's slot_base is added).  The lists stay resident next to the plan's descriptors; from then on
 * bce_plan_run_step(s) and the graph of bce_plan_run launch the check after the kernels of step s, with tag = s.  A plan
 * that was already captured is captured again at its next bce_plan_run.  All sizes 0 (or check_sizes NULL) detaches. */
int bce_plan_set_checks(bce_ctx*, bce_plan*, const uint32_t* check_sizes /*[n_steps]*/, const uint32_t* slots, int repair);
/* The expected bits of the next run(s), expect[instances][sum(check_sizes)], copied into one fixed device buffer of the
 * plan (a captured graph stays valid from one run to the next).  A plan with checks that is run before this call:
 * BCE_ERR_STATE. */
int bce_plan_set_expected(bce_ctx*, bce_plan*, const uint8_t* expect);
int bce_check_reset(bce_ctx*);
/* synchronises; log (may be NULL with log_cap 0) receives min(report->log_count, log_cap) entries, in no particular order;
 * report->log_count = entries the device logged (<= BCE_CHECK_LOG_CAP) */
int bce_check_get(bce_ctx*, bce_check_report*, bce_check_entry* log, uint32_t log_cap);

/* ---- the hot path, dependency-driven ------------------------------------------------------------------
 * The reference alternates Circuit::_ManageGates (a gate is ready when every input wire has arrived,
 * src/circuit.cpp:575-683) with Circuit::_ExecuteGates (src/circuit.cpp:685-817) once per frontier.  A bce_dag
 * hands the engine the WHOLE bootstrap DAG of a circuit instead: `tasks` are bootstrapped gates in topological
 * order, in SSA form (every `out` slot is written by exactly one task and only read by later ones; inputs no
 * task writes are primary inputs).  bce_dag_run evaluates `instances` input sets `slot_stride` slots apart in ONE
 * persistent kernel launch: dependency counters and ready queues live in device memory, a workgroup that finishes a
 * bootstrap releases its consumers, idle workgroups pull the next ready bootstrap -- no kernel boundary and no
 * device-wide barrier between dependent gates.  Every register holds the same ciphertext as under
 * bce_eval_gates_strided called frontier by frontier.  `prio` (may be NULL) gives each task a priority class
 * 0 (most urgent) .. 3; ready tasks of a lower class number are pulled first.
 * Asynchronous like bce_eval_gates; a run in which the device scheduler made no progress for the stall limit
 * (bce_dag_set_limits) abandons its queues and the next synchronising call returns BCE_ERR_STATE. */
typedef struct bce_dag bce_dag;
int bce_dag_supported(const bce_ctx*);   /* 1 when this context's parameter class has the persistent kernel */
int bce_dag_create(bce_ctx*, uint32_t n_tasks, const bce_gate_desc* tasks, const uint8_t* prio, bce_dag** out);
/* The same, with pair descriptors (BCE_PAIR) among the tasks.  A pair task is ONE task with two outputs: the persistent
 * kernel runs its blind rotation once and the tail twice, and publishes `out` and `out + 1` with one release.  Both slots
 * obey the SSA rule (written by this task alone, read by later tasks only) and count for the slot range that bce_dag_run
 * checks against slot_stride (BCE_ERR_ARG) and the pool (BCE_ERR_POOL).  A later task that reads either output, or both,
 * depends on the pair once.  A pair counts as one bootstrap in bce_timing and bce_dag_last_run and as one level of the
 * DAG's depth.  Illegal bits 8.. of `op`: BCE_ERR_ARG, as in bce_eval_gates.  Plain task lists give the same DAG as
 * bce_dag_create. */
int bce_dag_create_pairs(bce_ctx*, uint32_t n_tasks, const bce_gate_desc* tasks, const uint8_t* prio, bce_dag** out);
/* instance k of a run uses the DAG's slot numbers shifted by slot_base + k * slot_stride */
int bce_dag_run(bce_ctx*, bce_dag*, uint32_t instances, uint32_t slot_stride, uint32_t slot_base);
void bce_dag_destroy(bce_ctx*, bce_dag*);
/* Checks attached to a DAG (verify mode on the dataflow schedule): check i belongs to task tasks[i] (distinct indices into
 * the DAG's task list).  From then on the workgroup that ran such a task decrypts the task's `out` register when the
 * bootstrap has finished, compares it with the expected message and, with repair != 0, replaces a wrong one BEFORE it
 * releases the task's consumers -- the point at which the reference's Gate::Evaluate does it (src/gate.cpp:153-160); no
 * extra launch.  Report and log: the context's block, bce_check_reset / bce_check_get, as for plans; a log entry carries
 * tag = task index, index = check number.  A check on a pair task (bce_dag_create_pairs) checks its FIRST output `out`;
 * second outputs are temporaries and cannot be named.  n_checks == 0 detaches.  Synchronises.  BCE_ERR_NO_KEYS without keys,
 * BCE_ERR_ARG for a task index >= n_tasks, a duplicate task index or a null pointer. */
int bce_dag_set_checks(bce_ctx*, bce_dag*, uint32_t n_checks, const uint32_t* tasks /*[n_checks], distinct*/, int repair);
/* The expected messages (0..3) of the next run(s) of `instances` instances, expect[instances][n_checks]; asynchronous
 * (pinned staging, stream order).  BCE_ERR_ARG for a value above 3 or a null pointer, BCE_ERR_STATE for a DAG without
 * checks.  bce_dag_run on a DAG with checks: BCE_ERR_STATE before this call, or with another `instances` than it named. */
int bce_dag_set_expected(bce_ctx*, bce_dag*, uint32_t instances, const uint8_t* expect /*[instances][n_checks]*/);
/* workgroups_per_cu: 0 = choose by the work per dependency level, 1 or 2 = force; placement: 1 = idle compute
 * units claim ready bootstraps first (default), 0 = first poller wins; lazy_us: how long a half-busy compute unit
 * leaves a short queue to idle ones; stall_ms: no completion anywhere for this long abandons the run. */
int bce_dag_set_limits(bce_ctx*, int workgroups_per_cu, int placement, uint32_t lazy_us, uint32_t stall_ms);
/* counters of the last finished bce_dag_run (after a synchronising call): out[0] bootstraps completed,
 * out[1] claims a half-busy compute unit delayed in favour of an idle one, out[2] abort code (0 = none),
 * out[3] workgroups per CU the run used, out[4] / out[5] 100 MHz ticks summed over all workgroups between claiming
 * a bootstrap and releasing its consumers / spent looking for a bootstrap they then got, out[6] ticks spent waiting at the
 * XCD start gates (inside out[4]) */
int bce_dag_last_run(bce_ctx*, uint64_t out[7]);
/* test hook: task `t` of the DAG waits for one producer more than it has, so it never becomes ready and the run
 * stalls (exercises the bounded-spin exit) */
int bce_dag_debug_block_task(bce_dag*, uint32_t t);

/* ---- measurement ------------------------------------------------------- */
int bce_timing_reset(bce_ctx*);
int bce_timing_get(bce_ctx*, bce_timing* out); /* synchronizes */
/* on (default): every blind-rotation / tail launch carries a start and a stop timestamp ON ITS OWN DISPATCH (hipExtLaunchKernel
 * events: the *_ms fields are the kernels' own durations, nothing is recorded between dependent kernels; 11 us per dependent step
 * on the device timeline against 15.6 us with events recorded around the launches, as rounds 1-2 did).  off: launches and
 * bootstraps are still counted, the *_ms fields stop growing, plain launches.  bce_dag_run / bce_plan_run keep their one pair. */
int bce_timing_set_events(bce_ctx*, int on);
/* algorithmic bytes one gate-bootstrap reads at the widths this engine ships
 * (SURVEY.md 8(d) formula with w_bsk, w_ks, w_ct of this build) */
uint64_t bce_bytes_per_bootstrap(const bce_ctx*);
/* the same figure split by the kernel that moves the bytes: out[0] = bootstrapping-key rows (blind rotation),
 * out[1] = key-switching-key rows (tail gather), out[2] = ciphertext input / output words */
int bce_bytes_per_bootstrap_parts(const bce_ctx*, uint64_t out[3]);
/* forward transforms one AddToAcc step runs: 2 dG as in the reference (rgsw-acc-cggi.cpp / rgsw-acc-dm.cpp AddToAcc),
 * or 2 dG - 2 when this context keeps its key with the lowest gadget digit folded in (same accumulator words; the
 * decomposition is exact for the parameter set and the digit-0 rows multiply the accumulator itself) */
uint32_t bce_forward_transforms_per_step(const bce_ctx*);
/* 1 when saturated launches of this context run their forward transforms as quarter units, three per wave (folded
 * N = 1024 GINX kernel at two workgroups per compute unit, even 2N / q); 0: whole-row + half-row bodies (other contexts,
 * or BCE_FWD_UNITS=0 at context creation). */
uint32_t bce_forward_units(const bce_ctx*);
/* 1 when those quarter units run the stages on position bits 9..4 on the matrix pipe: i8 products of the gadget digits with
 * the four 7-bit limbs of one constant 64 x 64 matrix (needs the quarter units, gadget base <= 2^7 and the bounds of
 * csrc/fwd_mfma.hpp for this Q); 0: the quarter-unit body, in other contexts or with BCE_FWD_MFMA=0 at context creation. */
uint32_t bce_forward_mfma(const bce_ctx*);
/* 1 when the context was granted the lazy arithmetic of the 32-bit kernels (forward transforms without corrections, 64-bit
 * MAC sums, Montgomery MAC tail: the bounds ok1..ok5 of derive_params, csrc/ctx_params.cpp, hold for this Q, N and digit count);
 * 0: the corrected forms.  Always 1 for Q >= 2^28 (the 64-bit kernels have one form).  Read-only; for tests that look for the
 * largest modulus of a class. */
uint32_t bce_lazy_arithmetic(const bce_ctx*);
/* The host-built tables of that body, without a context or a device (tests).  Any output pointer may be null.
 * psi: the 2N-th root used; M6[64][64]: the six stages as a matrix over the positions p >> 4; C[64]: the balance words of
 * the raw-digit form (the kernel multiplies signed digits and needs none); table[4096]: the device image (A operands per
 * quarter, tile and lane); w14: 2^14 mod Q and its Shoup companion; bounds[4]: limb sum, low part, high part, recombined word.
 * Returns 1: the body may be enabled for these parameters; -1: tables built but a bound fails; 0: not this class
 * (N != 1024, dG != 4, gBits > 7, Q >= 2^28 or Q != 1 mod 2N), nothing written. */
int bce_forward_mfma_tables(uint64_t Q, uint32_t N, uint32_t gBits, uint32_t dG, uint64_t* psi, uint32_t* M6, uint32_t* C,
                            uint32_t* table, uint32_t* w14, uint64_t* bounds);
/* Launch granularity of this context's blind-rotation kernels, for callers that shape their frontiers (the host
 * scheduler of bce_circuit.h does): one bootstrap is one workgroup, so a call's time is a staircase in its size.
 * *lone = bootstraps up to which every workgroup has a compute unit to itself (one bootstrap latency per call),
 * *full = bootstraps resident at once when the device is saturated (each further multiple costs one more round). */
int bce_launch_capacity(const bce_ctx*, uint32_t* lone, uint32_t* full);

/* ---- what a context would decide, without a context or a device --------- */
/* The derivation bce_ctx_create* runs (csrc/ctx_params.cpp), for `cu_count` compute units and the context knobs of the
 * environment: one 64-bit value per item.  BCE_D_n .. BCE_D_w14s are the scalar fields of the kernels'
 * parameter block under their own names (doubles as their bit patterns), then: the per-XCD counters are wanted, the 2N-th
 * root, the granted kernel class (family: 0 one wave per transform, 1 split transform, 2 64-bit integer, 3 doubles), what
 * bce_launch_capacity, bce_bytes_per_bootstrap_parts and bce_forward_transforms_per_step would answer, FNV-1a-64 digests of
 * the host tables' bytes, and the LDS bytes of one workgroup of the persistent kernel's two-per-CU build (0 for Q >= 2^28).
 * Returns the status bce_ctx_create* would return on a machine with a device (never BCE_ERR_NO_DEVICE); *message (may be
 * NULL) receives the text bce_last_error would hold, "" for BCE_OK; `out` is all zero unless BCE_OK. */
enum { BCE_D_n = 0, BCE_D_N, BCE_D_logN, BCE_D_q, BCE_D_Q, BCE_D_qKS, BCE_D_baseKS, BCE_D_dKS, BCE_D_ksk_stride, BCE_D_ksk_u16,
       BCE_D_ks_chunk, BCE_D_gBits, BCE_D_dG, BCE_D_baseR, BCE_D_dR, BCE_D_method_ap, BCE_D_factor, BCE_D_Q8p1, BCE_D_red_shift,
       BCE_D_red_mu, BCE_D_Ninv, BCE_D_Ninv_s, BCE_D_Winv_last, BCE_D_Winv_last_s, BCE_D_mu32, BCE_D_lazy, BCE_D_c32,
       BCE_D_occupancy_target, BCE_D_variant, BCE_D_cu_count, BCE_D_xcd_gate_ticks, BCE_D_fuse_tail, BCE_D_fold_ninv, BCE_D_fold,
       BCE_D_fwd_units, BCE_D_factor_even, BCE_D_I4_0, BCE_D_I4_1, BCE_D_I4_2, BCE_D_I4_3, BCE_D_I4s_0, BCE_D_I4s_1, BCE_D_I4s_2,
       BCE_D_I4s_3, BCE_D_qinv_neg, BCE_D_r2_off, BCE_D_is64, BCE_D_Q64, BCE_D_Q8p1_64, BCE_D_mu64, BCE_D_c64, BCE_D_Ninv64,
       BCE_D_Ninv64_s, BCE_D_fp64, BCE_D_Qd, BCE_D_invQd, BCE_D_Ninvd, BCE_D_Ninvd_q, BCE_D_pool_stride, BCE_D_fwd_mfma, BCE_D_w14,
       BCE_D_w14s,
       BCE_D_xcd_gate, BCE_D_psi,
       BCE_D_family, BCE_D_fold_build, BCE_D_dag, BCE_D_wg_per_cu_lone, BCE_D_wg_per_cu_full, BCE_D_lds_bytes,
       BCE_D_capacity_lone, BCE_D_capacity_full, BCE_D_bytes_bsk, BCE_D_bytes_ksk, BCE_D_bytes_ct, BCE_D_forward_transforms,
       BCE_D_fnv_twf, BCE_D_fnv_psi, BCE_D_fnv_psi_r2, BCE_D_fnv_tw64, BCE_D_fnv_tw64d, BCE_D_fnv_fwd_mfma,
       BCE_D_dag_lds_bytes, BCE_D_COUNT };
int bce_params_derive(uint32_t n, uint32_t N, uint64_t q, uint64_t Q, uint64_t qKS, uint32_t baseKS, uint32_t baseG, uint32_t baseR,
                      int method, uint32_t cu_count, uint64_t out[BCE_D_COUNT], const char** message);
/* the same for a tabulated set (enum bce_paramset) */
int bce_params_derive_set(int paramset, int method, uint32_t cu_count, uint64_t out[BCE_D_COUNT], const char** message);
/* What bce_dag_run would launch for a context with the report `derived` (of the two entries above), the limits of
 * bce_dag_set_limits, a DAG whose longest chain has `depth` tasks and `items` = tasks x instances bootstraps, under the DAG
 * knobs of the environment: out[BCE_L_wps] 2 = one workgroup per compute unit, 4 = two (bce_dag_last_run's out[3] is half of
 * it); the grid; the policy bits, gate and timeout words the device scheduler receives; re-arm only (development). */
enum { BCE_L_wps = 0, BCE_L_grid, BCE_L_policy, BCE_L_gate_ticks, BCE_L_gate_backlog, BCE_L_lazy_ticks, BCE_L_stall_ticks,
       BCE_L_rearm_only, BCE_L_COUNT };
int bce_dag_launch_choice(const uint64_t derived[BCE_D_COUNT], int workgroups_per_cu, int placement, uint32_t lazy_us,
                          uint32_t stall_ms, uint32_t depth, uint64_t items, uint64_t out[BCE_L_COUNT]);

/* ---- in-library collective (multi-GPU, one process per GPU) ---------------------------------------------
 * RCCL all-gather issued on the engine's own stream, so that the exchange of boundary ciphertexts between two
 * dependent frontiers needs neither a host synchronisation nor the host language (bce_circuit_enable_rccl uses
 * it).  RCCL is dlopen()ed on first use.  Rendezvous: rank 0 calls bce_rccl_unique_id and the host program
 * delivers the 128 bytes to every rank, each of which then calls bce_rccl_init with its rank. */
int bce_rccl_available(void);   /* 1 when the RCCL library and the entry points used here could be loaded */
int bce_rccl_version(void);     /* ncclGetVersion of that library (2.x ABI required), 0 if none.  NOTE: between two or more
                                 * devices this path has not run on hardware yet (no multi-GPU node was available to the
                                 * builder); the torch.distributed callback of bce_circuit_set_exchange is the verified one. */
int bce_rccl_unique_id(uint8_t out[128]);
int bce_rccl_init(bce_ctx*, const uint8_t uid[128], int rank, int world);
/* every rank contributes `bytes` bytes at dev_send and receives world * bytes at dev_recv, rank-major; asynchronous,
 * ordered with the engine's kernels */
int bce_rccl_allgather(bce_ctx*, const void* dev_send, void* dev_recv, uint64_t bytes);
int bce_rccl_shutdown(bce_ctx*);
/* what the context's communicator reports: out[0] = ncclCommCount (ranks RCCL sees), out[1] = ncclCommUserRank,
 * out[2] = ncclCommCuDevice.  Lets a caller (bench.py, tests) prove what the exchange collective spans. */
int bce_rccl_comm_info(bce_ctx*, int out[3]);

/* ---- staged outputs for parity tests ----------------------------------- */
/* Runs the frontier like bce_eval_gates and also returns the intermediates
 * (any pointer may be NULL): acc = accumulator after blind rotation,
 * COEFFICIENT domain, u64 [n_desc][2][N]; lweN = after extract + ModSwitch(Q->qKS),
 * u64 [n_desc][N+1]; ks = after KeySwitch, u64 [n_desc][n+1].  Bootstrapped ops only.
 * With P pair descriptors (BCE_PAIR) lweN and ks have n_desc + P rows: rows [0, n_desc) are the first outputs, the second
 * outputs follow from row n_desc on in descriptor order; acc stays one (shared) accumulator per descriptor. */
int bce_debug_eval_stages(bce_ctx*, uint32_t n_desc, const bce_gate_desc* descs, uint64_t* acc,
                          uint64_t* lweN, uint64_t* ks);
/* The tail of EvalBinGate alone on caller-supplied accumulators: acc = u64 [count][2][N], COEFFICIENT domain, words < Q
 * (what `acc` of bce_debug_eval_stages returns).  Runs transpose + extract (a = coefficients of acc[0](X^-1),
 * b = acc[1][0] + Q/8 + 1), ModSwitch(Q -> qKS), KeySwitch, ModSwitch(qKS -> q) -- lbcrypto::LWEEncryptionScheme::
 * ModSwitch / KeySwitch as BinFHEScheme::EvalBinGate calls them after the accumulator -- and writes the refreshed
 * ciphertexts to pool slots out_slots[count]; lweN / ks (may be NULL) as in bce_debug_eval_stages.  Used by
 * tools/openfhe_export/compare.py to replay OpenFHE's own tail records (kind BCE_GATEVEC_TAIL of bce_keyfile.h). */
int bce_debug_tail(bce_ctx*, uint32_t count, const uint64_t* acc, const uint32_t* out_slots, uint64_t* lweN,
                   uint64_t* ks);
/* Workgroups the separate tail kernels spread ONE bootstrap's key-switch rows over in a launch of `count` bootstraps
 * (16, 8, 4, 2 or 1: the rule launch_tail itself applies).  Read-only; for tests that must know which split a launch ran. */
uint32_t bce_debug_tail_split(const bce_ctx*, uint32_t count);
/* forward (inverse=0) / inverse negacyclic NTT of `count` polys, in place, u64 [count][N];
 * forward output is in the engine's internal evaluation order. */
int bce_debug_ntt(bce_ctx*, uint64_t* polys, uint32_t count, int inverse);

#ifdef __cplusplus
}
#endif
#endif
