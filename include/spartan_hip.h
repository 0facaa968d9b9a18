/* spartan_hip — MI355X-native drop-in for the proving hot path of tsunrise/r1cs-spartan.
 *
 * C ABI of libspartan_hip.so. Every entry point returns an spx_status; on failure
 * spx_last_error() holds a thread-local message. No torch / HIP types cross this boundary:
 * plain pointers, sizes and byte images.
 *
 * Byte conventions (ark-serialize, the reference's own wire format):
 *   Fr        32-byte little-endian canonical integer (`into_repr` bytes)
 *   G1 / G2   96 / 192-byte UNCOMPRESSED affine points (spx_pp_load / spx_pp_serialize, every
 *             VerifierParameter argument), 48 / 96-byte COMPRESSED points inside proofs and in the
 *             compressed public-parameter form (spx_pp_load_compressed / spx_pp_serialize_compressed;
 *             spx_vp_convert takes a VerifierParameter from one form to the other)
 *   Matrix    CSR: row_ptr[n+1] (u64), col[nnz] (u32), val[nnz] (Fr bytes); the row order and
 *             the order of entries inside a row are the `ark_relations::r1cs::Matrix<F>` order
 *             (they are hashed into the Fiat-Shamir transcript, /root/reference/src/lib.rs:61-64).
 *
 * Reference interfaces replaced (file:line in /root/reference):
 *   spx_index            MLArgumentForR1CS::index                 src/lib.rs:45-51 -> src/ahp/indexer.rs:41-64
 *   spx_prove            MLArgumentForR1CS::prove                 src/lib.rs:58-146
 *   spx_verify           MLArgumentForR1CS::verify                src/lib.rs:147-212
 *   spx_pp_load          PublicParameter::deserialize_unchecked of serialize_uncompressed bytes  src/commitment/data_structures.rs:9-17
 *   spx_pp_serialize     PublicParameter::serialize_uncompressed
 *   spx_pp_load_compressed       PublicParameter::deserialize (CanonicalDeserialize's default, compressed;
 *                                with spx_pp_check_subgroup: the checked deserialize)
 *   spx_pp_serialize_compressed  PublicParameter::serialize (CanonicalSerialize's default, compressed)
 *   spx_vp_convert       VerifierParameter::serialize <-> serialize_uncompressed bytes
 *   spx_pp_generate      MLProofForR1CS::setup / MLPolyCommit::keygen  src/ahp/setup.rs:13-16, src/commitment/setup.rs:27-105
 *   spx_commit           MLPolyCommit::commit                     src/commitment/commit.rs:17-29
 *   spx_open             MLPolyCommit::open                       src/commitment/open.rs:19-58
 *   spx_pc_verify        MLPolyCommit::verify                     src/commitment/verify.rs:12-45
 *   spx_sum_over_y       MatrixExtension::sum_over_y              src/data_structures/r1cs_reader.rs:75-85
 *   spx_eval_on_x        MatrixExtension::eval_on_x               src/data_structures/r1cs_reader.rs:91-117
 *   spx_msm_g1 / _g2     ark-ec VariableBaseMSM::multi_scalar_mul (called at commit.rs:25, open.rs:49)
 *   spx_prover_*, spx_prove_*_round   the round-level prover API  src/ahp/prover.rs:109-281
 *   spx_sumcheck_round   AHPForMLSumcheck::prove_round [linear-sumcheck] (called at prover.rs:204, 263)
 * Errors mirror src/error.rs:5-14 (Display is todo!() there; here a message string).
 */
#ifndef SPARTAN_HIP_H
#define SPARTAN_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    SPX_OK = 0,
    SPX_INVALID_ARGUMENT = 1, /* Error::InvalidArgument */
    SPX_SUMCHECK = 2,         /* Error::SumCheckError */
    SPX_WRONG_WITNESS = 3,    /* Error::WrongWitness */
    SPX_SERIALIZATION = 4,    /* Error::SerializationError */
    SPX_DEVICE = 5            /* HIP / RCCL failure (no reference counterpart) */
} spx_status;

typedef struct spx_ctx spx_ctx;         /* one GPU (one rank): stream, workspaces, communicator */
typedef struct spx_pp spx_pp;           /* device-resident public parameters (+ window tables) */
typedef struct spx_pk spx_pk;           /* prover key (IndexPK): matrices on host (transcript) and device */
typedef struct spx_witness spx_witness; /* z = v || w resident in HBM */

typedef struct {
    uint64_t n;               /* rows (= number of constraints) */
    const uint64_t *row_ptr;  /* n + 1 */
    const uint32_t *col;      /* nnz */
    const uint8_t *val;       /* 32 * nnz */
} spx_csr;

typedef enum { SPX_FS = 0, SPX_INJECTED = 1 } spx_mode;

typedef struct {
    int mode;            /* SPX_FS: Blake2s512Rng Fiat-Shamir (reference); SPX_INJECTED: SplitMix64(inj_seed) */
    uint64_t inj_seed;
    int cached_matrix_transcript; /* 1: resume the Blake2s state absorbed at spx_index time (bit-identical) */
    int commitment_stub; /* 1: BASELINE config C2, "sumcheck-only, commitment stubbed": the proof prove()
                            gives under a public parameter whose every group element is the identity
                            (commitment, h and opening proofs = infinity; the z evaluations are still
                            computed). No MSM runs and pp may be NULL. Not a sound proof: benchmark /
                            parity mode of the sumcheck half of lib.rs:58-146. */
} spx_prove_opts;

const char *spx_last_error(void);
const char *spx_version(void);

/* ---- context / multi-GPU ---- */
int spx_ctx_create(int device, spx_ctx **out);
int spx_ctx_destroy(spx_ctx *ctx);
/* RCCL (one process per GPU): rank 0 calls spx_comm_unique_id, broadcasts the 128 bytes out of band
 * (e.g. torch.distributed), then every rank creates ONE hub on it (spx_comm_hub_create_rccl) and
 * attaches each of its contexts to a channel (spx_ctx_set_comm_hub): context j of every rank on
 * channel j (0..63). The hub's thread is the only caller of the communicator and matches the
 * channels' exchanges across ranks in rounds every rank runs identically, so any number of proofs in
 * flight share one communicator without collective-ordering deadlocks.
 * spx_ctx_set_comm_rccl is the one-context shorthand (a private hub, channel 0).
 * Replaces the reference's single-threaded prove (/root/reference/src/lib.rs:58-146), which has
 * no exchange; the exchange schedule is DESIGN.md §6. */
int spx_comm_unique_id(uint8_t id_out[128]);
int spx_ctx_set_comm_rccl(spx_ctx *ctx, const uint8_t id[128], int rank, int world);
int spx_comm_hub_create_rccl(const uint8_t id[128], int rank, int world, int device, void **hub_out);
/* the same hub over the shared-memory transport (one segment per rank set instead of one per
 * context), and over the in-process test group (virtual ranks as host threads; spx_comm_group_create) */
int spx_comm_hub_create_shm(const char *name, int rank, int world, void **hub_out);
int spx_comm_hub_create_group(void *group, int rank, void **hub_out);
/* ... and over a caller-provided collective (e.g. a torch.distributed process group: gloo on the CPU,
 * RCCL = backend "nccl" on MI355X): fn(user, send, recv, bytes) must gather `bytes` from every rank of
 * the caller's group into recv in rank order and return 0 (non-zero fails the exchange with
 * SPX_DEVICE); rank / world are the caller's group's. Only the hub's thread calls fn, in the same
 * sequence on every rank. */
typedef int (*spx_allgather_fn)(void *user, const void *send, void *recv, size_t bytes);
int spx_comm_hub_create_callback(spx_allgather_fn fn, void *user, int rank, int world, void **hub_out);
int spx_ctx_set_comm_hub(spx_ctx *ctx, void *hub, int channel);
/* one exchange on `channel` without a context (transport tests); blocks until every rank posted it */
int spx_comm_hub_allgather(void *hub, int channel, const void *send, void *recv, size_t bytes);
/* out[0] control rounds, out[1] data rounds, out[2] exchanges served, out[3] largest batch per round,
 * out[4] idle rounds (matched nothing: a peer had not reached the exchange yet; each is followed by a
 * 50 us back-off or the next local request) */
int spx_comm_hub_stats(void *hub, uint64_t out[5]);
int spx_comm_hub_destroy(void *hub); /* contexts attached keep the hub alive until they are destroyed */
/* On-node shared-memory communicator (default for one process per GPU on one host): every rank
 * passes the same `name` (rank 0 makes it unique, e.g. "spx_<random hex>_<k>", and distributes it
 * out of band), one name per context. The exchanges of a sharded proof are host-side and tiny, so
 * no GPU queue is involved (multi-GPU). The standalone form is a host-only
 * allgather (tests, other transports' validation). */
int spx_ctx_set_comm_shm(spx_ctx *ctx, const char *name, int rank, int world);
int spx_comm_shm_create(const char *name, int rank, int world, void **comm_out);
int spx_comm_shm_allgather(void *comm, const void *send, void *recv, size_t bytes);
int spx_comm_shm_destroy(void *comm);
/* In-process test communicator: `world` contexts sharing one exchange object (shards of one proof
 * driven by `world` host threads). group_create returns a handle; each ctx joins with its rank. */
int spx_comm_group_create(int world, void **group_out);
int spx_comm_group_destroy(void *group);
int spx_ctx_set_comm_group(spx_ctx *ctx, void *group, int rank);
/* Rehearsal: this context acts as rank `rank` of a `world`-rank proof-sharded prove WITHOUT peers
 * (every exchange returns its own contribution in all slots): the device and host work of one rank
 * on a GPU of its own, for throughput estimates of an N-GPU node. Its proofs are not valid. */
int spx_ctx_set_comm_rehearsal(spx_ctx *ctx, int rank, int world);
/* Where the shared level-0 opening MSM of a proof runs (no effect on the proof bytes): 0 = beside the
 * commitment (its own MSM pipeline, the default), 1 = inside the first opening's MSM batch (one MSM
 * pipeline less per proof: sort, weighting tree), -1 = the process default (SPX_LVL0=batch -> 1).
 * Every rank of a proof-sharded prove must use the same mode (checked on the context's first sharded
 * proof: SPX_INVALID_ARGUMENT otherwise). */
int spx_ctx_set_lvl0_batch(spx_ctx *ctx, int mode);
/* Hot-bucket reduction of this context's MSMs (no effect on the proof bytes): a bucket that the
 * planned partial levels leave with more than 4 partials (skewed scalars: a 0 / 1 witness sends every
 * 1 to one bucket) is reduced by a parallel tree before the bucket weighting. 1 = on (the default),
 * 0 = off (such buckets are still listed and counted, then added serially by the weighting leaf: A/B),
 * -1 = the process default (SPX_MSM_HOT=0 -> 0, else 1). Each rank of a proof-sharded prove may choose
 * its own. SPX_INVALID_ARGUMENT while the context is in use. */
int spx_ctx_set_msm_hot(spx_ctx *ctx, int mode);
/* one allgather on the context's communicator (whatever its transport): every rank passes `bytes`,
 * recv receives world * bytes in rank order. For transport tests. */
int spx_ctx_comm_allgather(spx_ctx *ctx, const void *send, void *recv, size_t bytes);

/* How this context's host waits for its stream (no effect on the proof bytes): us > 0 polls an event
 * every us microseconds (frees the host cores the HSA runtime's spinning wait would take: BASELINE C2
 * with matrices absorbed per proof, sharded ranks), 0 = hipStreamSynchronize, -1 = the process default
 * (SPX_SYNC_POLL_US, else 0). */
int spx_ctx_set_sync_poll(spx_ctx *ctx, int us);
/* Lockstep groups for spx_prove_many (no effect on the proof bytes): with k > 1 (at most 16) the
 * context's stubbed-commitment proofs on an unsharded context (BASELINE C2) run k at a time in
 * lockstep: each sumcheck round of the k proofs is one launch (blockIdx.y = proof) with one host wait,
 * and the other steps queue the k proofs' launches before one wait. Other proofs, and
 * k = 1 (the default), run one at a time. Replaces nothing in the reference (its prove is one proof,
 * /root/reference/src/lib.rs:58-146); each proof's bytes are that prove's. */
int spx_ctx_set_group(spx_ctx *ctx, int k);
/* free and total bytes of the context's device (hipMemGetInfo): bench.py sizes the proofs in flight
 * per rank from it (each context keeps grow-only scratch and an MSM workspace) */
int spx_ctx_mem_info(spx_ctx *ctx, uint64_t *free_bytes, uint64_t *total_bytes);

/* ---- public parameters ---- */
int spx_pp_load(spx_ctx *ctx, const uint8_t *bytes, size_t len, spx_pp **out);
int spx_pp_generate(spx_ctx *ctx, int nv, uint64_t seed, spx_pp **out);
int spx_pp_serialize(spx_pp *pp, uint8_t *out, size_t cap, size_t *len);
/* The compressed wire form: what `pp.serialize(&mut w)` writes and `PublicParameter::deserialize` reads
 * (ark-serialize's default methods). The framing is that of the uncompressed form in the derive order of
 * data_structures.rs:9-17 (u64 nv, u64 nv, per G1 level u64 2^(nv-i) and its points, u64 nv, per G2 level
 * likewise, g, h) with 48-byte G1 and 96-byte G2 points: half the bytes to store and to move over PCIe.
 *
 * spx_pp_load_compressed: the points are decompressed on the GPU straight into the parameter's device
 * layout, with the acceptance of spx_g1_decompress / spx_g2_decompress; then the handle is preprocessed as
 * spx_pp_load's and cannot be told apart from one (views, derived VP, checks, window plans, memory).
 * Framing errors give spx_pp_load's messages. A rejected point gives SPX_SERIALIZATION naming the lowest
 * offender in the order of spx_pp_check_subgroup (G1 levels, G2 levels, g, h), e.g.
 * "powers_of_h level 2 point 5: x is not canonical" or "...: no point on the curve with this x".
 * The bytes are uploaded through a device staging buffer in chunks of at most 2^SPX_PP_STAGE_LOG points
 * (environment, read at each call; default 20: at most 96 MiB of staging whatever the size).
 * spx_pp_serialize_compressed: the contract of spx_pp_serialize (len receives the size; SPX_INVALID_ARGUMENT
 * if cap is too small) for loaded and generated parameters and views, staged in the same chunks.
 * spx_pp_serialized_size: the byte length of an nv-variable parameter (1..26) in either form; host only. */
int spx_pp_load_compressed(spx_ctx *ctx, const uint8_t *bytes, size_t len, spx_pp **out);
int spx_pp_serialize_compressed(spx_pp *pp, uint8_t *out, size_t cap, size_t *len);
int spx_pp_serialized_size(int nv, int compressed, size_t *len);
/* A VerifierParameter (u64 nv, g, h, u64 count, g_mask_random) from the uncompressed form, which
 * spx_verify / spx_verify_many / spx_pc_verify take, to the compressed one (to_compressed = 1) or back
 * (0), on the host: a Rust host passes `vp.serialize()` through this call first. Malformed input
 * (truncated, trailing bytes, a non-canonical x, an x with no point) gives SPX_SERIALIZATION. */
int spx_vp_convert(const uint8_t *in, size_t in_len, int to_compressed, uint8_t *out, size_t cap, size_t *len);
int spx_pp_free(spx_pp *pp);

/* ---- index / witness / prove ---- */
int spx_index(spx_ctx *ctx, const spx_csr *a, const spx_csr *b, const spx_csr *c, spx_pk **out);
int spx_index_free(spx_pk *idx);
/* Who builds the device layouts of this context's indices (no effect on the arrays, and so none on any
 * proof): 0 = the host builder (the default), 1 = the GPU builder: each matrix is uploaded once, its
 * values converted to Montgomery form once, and HIP kernels make the row layout (CSR block or
 * column-sorted list), the last-entry-wins CSC and the column stream while the calling thread absorbs
 * A, B, C into the cached transcript; -1 = the process default (SPX_INDEX_BUILD=gpu -> 1, else 0). The
 * host-side checks of the matrices, their statuses and messages are the same. The GPU builder takes
 * fewer than 2^31 entries in A, B and C together (SPX_INVALID_ARGUMENT otherwise). Each rank of a
 * proof-sharded prove may choose its own. SPX_INVALID_ARGUMENT while the context is in use. */
int spx_ctx_set_index_build(spx_ctx *ctx, int mode);
/* Diagnostic: the raw bytes of one device array of an index (values in the device's Montgomery form:
 * 8 32-bit limbs, least significant first). With out == NULL only *len is written. Lengths are the
 * logical ones; a part the index does not have (the sliced list of a CSR index and the reverse, the
 * long tables of an index without long rows or columns) has length 0. Element layouts: PTR uint64,
 * IDX / COL / DST / LANES / ROWM uint32, VAL 32 B, CHUNKS {u32 m, u32 0, u64 begin, u64 end},
 * LROWS {u32 m, u32 chunk_begin, u32 chunk_end, u32 0, u64 x}, SLICES {u64 off, u32 len, u32 0}. */
enum {
    SPX_IDX_ROWS_PTR_A = 0, SPX_IDX_ROWS_PTR_B, SPX_IDX_ROWS_PTR_C,
    SPX_IDX_ROWS_IDX_A, SPX_IDX_ROWS_IDX_B, SPX_IDX_ROWS_IDX_C,
    SPX_IDX_ROWS_VAL_A, SPX_IDX_ROWS_VAL_B, SPX_IDX_ROWS_VAL_C,
    SPX_IDX_ROWS_CHUNKS, SPX_IDX_ROWS_LROWS,
    SPX_IDX_SLICED_VAL, SPX_IDX_SLICED_COL, SPX_IDX_SLICED_DST,
    SPX_IDX_COLS_SLICES, SPX_IDX_COLS_LANES, SPX_IDX_COLS_ROWM, SPX_IDX_COLS_VAL,
    SPX_IDX_LONGC_IDX_A, SPX_IDX_LONGC_IDX_B, SPX_IDX_LONGC_IDX_C,
    SPX_IDX_LONGC_VAL_A, SPX_IDX_LONGC_VAL_B, SPX_IDX_LONGC_VAL_C,
    SPX_IDX_LONGC_CHUNKS, SPX_IDX_LONGC_LROWS,
    SPX_IDX_PART_COUNT
};
int spx_index_export(spx_pk *idx, int part, uint8_t *out, size_t cap, size_t *len);
/* out[0] the builder that made the index (0 host | 1 GPU), out[1] its row layout (1 = the column-sorted
 * list, 0 = CSR), out[2] entries of the row layout, out[3] live entries of the local columns (after
 * last-entry-wins), out[4] long rows (records of more than 64 entries), out[5] local columns of more
 * than 62 entries, out[6] wall microseconds of the whole spx_index call, out[7] microseconds of it
 * the calling thread spent absorbing A, B, C into the cached transcript. With the GPU builder,
 * spx_last_timings[0] after spx_index is the device time (us, HIP events) of its kernels. */
int spx_index_stats(spx_pk *idx, uint64_t out[8]);
int spx_witness_upload(spx_ctx *ctx, const uint8_t *v, size_t nv, const uint8_t *w, size_t nw, spx_witness **out);
int spx_witness_free(spx_witness *wit);
size_t spx_proof_size(int log_n, int log_v);
/* host buffers in, proof bytes out (the reference's prove(pk, v, w, &pp) -> Proof, serialized) */
int spx_prove(spx_ctx *ctx, spx_pk *idx, const uint8_t *v, size_t nv, const uint8_t *w, size_t nw, spx_pp *pp,
              const spx_prove_opts *opts, uint8_t *out, size_t cap, size_t *len);
/* witness already resident in HBM (the benchmarked form) */
int spx_prove_witness(spx_ctx *ctx, spx_pk *idx, spx_witness *wit, spx_pp *pp, const spx_prove_opts *opts,
                      uint8_t *out, size_t cap, size_t *len);
/* Proves nproofs witnesses of one index concurrently: worker k drives ctxs[k] (its own HIP stream,
 * MSM workspace and communicator) and proves witnesses k, k + nctx, ... in order. Every proof does
 * the complete per-proof work of spx_prove_witness (transcript absorption of A, B, C included unless
 * opts->cached_matrix_transcript). Proof i is written to out + i * stride, its length to lens[i].
 * All contexts must be on the device (and communicator rank) the index was built for. Throughput
 * form of lib.rs:58-146 for a prover serving many witnesses; returns the first failure's status. */
int spx_prove_many(spx_ctx **ctxs, int nctx, spx_pk *idx, spx_witness **wits, int nproofs, spx_pp *pp,
                   const spx_prove_opts *opts, uint8_t *out, size_t stride, size_t *lens);
/* ---- round-level prover: the reference's interactive API (src/ahp/prover.rs:109-281), driven with
 * verifier coins supplied by the caller as src/ahp/tests.rs:8-70 drives it. Each call takes the
 * verifier message of its step (canonical Fr, 32 B each) and returns the prover message, ark-serialize
 * compressed as the reference's message types (ProverFirstMessage .. ProverSixthMessage, the
 * linear-sumcheck ProverMsg / IndexInfo). The session runs the same kernels as spx_prove: with the
 * challenges a Fiat-Shamir prove would draw, the messages concatenate to spx_prove's proof (plus the
 * two sumchecks' u64 round counts). One session or prove per context at a time, enforced: from
 * spx_prover_init until the session's last round (or spx_prover_free) the context is claimed, and a
 * prove, verify, kernel-level call or second session on it fails with SPX_INVALID_ARGUMENT (so do
 * two concurrent proves on one context). Sessions need an unsharded context (comm size 1).
 *   spx_prover_init                  prover_init              prover.rs:109-121 (|v| power of two, |v|+|w| = n)
 *   spx_prover_first_round           prover_first_round       prover.rs:123-141 (commitment)
 *   spx_prover_second_round          prover_second_round      prover.rs:143-160 (r_v: log2|v| coins)
 *   spx_prover_third_round           prover_third_round       prover.rs:163-196 (tau: log_n coins)
 *   spx_prove_first_sumcheck_round   prove_first_sumcheck_round prover.rs:199-207 (NULL first, then r_{i-1})
 *   spx_prove_fourth_round           prove_fourth_round       prover.rs:210-228 (last point of r_x)
 *   spx_prove_fifth_round            prove_fifth_round        prover.rs:230-255 (r_a, r_b, r_c: 96 B)
 *   spx_prove_second_sumcheck_round  prove_second_sumcheck_round prover.rs:258-266 (NULL first, then r_{i-1})
 *   spx_prove_sixth_round            prove_sixth_round        prover.rs:268-281 (last point of r_y)
 * Out-of-order calls fail with SPX_INVALID_ARGUMENT; a sumcheck round given a challenge first, or
 * none later, or called past log_n rounds fails with SPX_SUMCHECK (linear-sumcheck's errors). */
typedef struct spx_prover spx_prover;
int spx_prover_init(spx_ctx *ctx, spx_pk *idx, const uint8_t *v, size_t nv, const uint8_t *w, size_t nw,
                    spx_prover **out);
int spx_prover_first_round(spx_prover *p, spx_pp *pp, uint8_t *msg, size_t cap, size_t *len);
int spx_prover_second_round(spx_prover *p, const uint8_t *r_v, size_t n, spx_pp *pp, uint8_t *msg, size_t cap,
                            size_t *len);
int spx_prover_third_round(spx_prover *p, const uint8_t *tau, size_t n, uint8_t *msg, size_t cap, size_t *len);
int spx_prove_first_sumcheck_round(spx_prover *p, const uint8_t *challenge, uint8_t *msg, size_t cap, size_t *len);
int spx_prove_fourth_round(spx_prover *p, const uint8_t *last_point, uint8_t *msg, size_t cap, size_t *len);
int spx_prove_fifth_round(spx_prover *p, const uint8_t *r_abc, uint8_t *msg, size_t cap, size_t *len);
int spx_prove_second_sumcheck_round(spx_prover *p, const uint8_t *challenge, uint8_t *msg, size_t cap, size_t *len);
int spx_prove_sixth_round(spx_prover *p, const uint8_t *last_point, spx_pp *pp, uint8_t *msg, size_t cap, size_t *len);
int spx_prover_free(spx_prover *p);

/* host time spent by spx_prove_many's hashing pools absorbing A, B, C (lib.rs:61-64), process-wide:
 * out[0] nanoseconds (summed over the pool threads), out[1] proofs absorbed, out[2] the multi-buffer
 * lane width (proofs hashed per vector instruction: 16 AVX-512, 8 AVX2, 1 scalar), out[3] nanoseconds
 * the proof workers waited for a proof's absorption (summed over the workers) */
int spx_hash_stats(uint64_t out[4]);
/* host CPU of the proving threads by prove() phase, process-wide since load: out[3 i], out[3 i + 1],
 * out[3 i + 2] = thread CPU ns, wall ns and count of phase i in the order transcript_matrices, commit,
 * open_rv, sumcheck1, eval_on_x, sumcheck2, open_ry (the phases of spx_last_timings) */
int spx_host_phase_stats(uint64_t out[21]);
/* MLArgumentForR1CS::verify (src/lib.rs:147-212, verifier.rs:143-512): SPX_OK = accepted (the
 * reference's Ok(true)); a rejection returns the reference's error kind (SPX_INVALID_ARGUMENT,
 * SPX_SUMCHECK, SPX_WRONG_WITNESS, SPX_SERIALIZATION) with its message in spx_last_error.
 * vp = VerifierParameter (commitment/data_structures.rs:19-26) in ark-serialize uncompressed form.
 * The matrix evaluation runs on the ctx's GPU; the index must be built on a single-rank context. */
int spx_verify(spx_ctx *ctx, spx_pk *idx, const uint8_t *v, size_t nv, const uint8_t *proof, size_t len,
               const uint8_t *vp, size_t vp_len, const spx_prove_opts *opts);
/* spx_verify for nproofs proofs of one index under one verifier parameter (lib.rs:147-212 per proof; the
 * mKZG checks, verify.rs:12-45, of the whole batch folded into one product of log_n + 2 pairings by a
 * random linear combination). v[j] / nv[j] / proofs[j] / lens[j]: proof j's public input
 * and bytes. entropy32: 32 bytes mixed into the coefficients, or NULL. status[j] receives what spx_verify
 * returns for proof j alone. Returns SPX_OK if every proof is accepted, otherwise the status of the
 * lowest-index rejected proof with that proof's message in spx_last_error. An error of the call itself
 * (a NULL, nproofs < 1, an index of a sharded context, a bad vp, a context in use) returns before
 * status[] is touched. The proofs' points are decompressed and combined on the ctx's GPU. */
int spx_verify_many(spx_ctx *ctx, spx_pk *idx, const uint8_t *const *v, const size_t *nv,
                    const uint8_t *const *proofs, const size_t *lens, int nproofs,
                    const uint8_t *vp, size_t vp_len, const spx_prove_opts *opts,
                    const uint8_t *entropy32 /* may be NULL */, int *status /* nproofs */);
/* the coefficients spx_verify_many takes for these arguments: out = 2 nproofs canonical Fr (32 B each),
 * rho_{j,o} at 2 j + o for proof j's opening o (0: at r_v, 1: at r_y). With seed = BLAKE2s-256 (RFC 7693,
 * unkeyed) of "spx-verify-many-v1" || vp || entropy32 (zeros if NULL) || for each proof LE64(nv_j) || v_j ||
 * LE64(len_j) || proof_j, rho_{j,o} = the low 128 bits (little-endian) of BLAKE2s-256(seed || LE64(2 j + o)),
 * or 1 if those are zero. Host only, no GPU. */
int spx_verify_many_coeffs(const uint8_t *const *v, const size_t *nv, const uint8_t *const *proofs,
                           const size_t *lens, int nproofs, const uint8_t *vp, size_t vp_len,
                           const uint8_t *entropy32 /* may be NULL */, uint8_t *out);
/* spx_verify_many on this context, cumulative: out[0] batches run (one combined pairing check each),
 * out[1] pairs given to the Miller loop by the batched path (log_n + 2 per batch), out[2] proofs sent to
 * the single-proof path, out[3] points decompressed on the GPU */
int spx_verify_stats(spx_ctx *ctx, uint64_t out[4]);
/* VerifierParameter of a keygen-generated PP (spx_pp_generate; setup.rs:91-101) or of a view of one,
 * from the trapdoor, uncompressed bytes. A loaded parameter has no trapdoor: use spx_pp_derive_vp. */
int spx_vp_from_pp(spx_pp *pp, uint8_t *out, size_t cap, size_t *len);
/* prod_i e(P_i, Q_i) == 1 over n pairs (uncompressed G1 96 B / G2 192 B each); host only, no GPU
 * (E::product_of_pairings as used by verify.rs:12-45) */
int spx_pairing_check(const uint8_t *g1, const uint8_t *g2, size_t n, int *is_one);
/* per-phase device timings of the last prove on this ctx, microseconds. After
 * spx_verify_many: host wall microseconds of its seven phases, in order (0 for one that did not run):
 * parse and transcript replay; points to the GPU with the algebraic checks; the wait for their
 * decompression; matrix evaluations; combinations; the pairing product; single-proof path */
int spx_last_timings(spx_ctx *ctx, double *out, int cap, int *n);

/* ---- R1CS front-end: ark-relations ConstraintSystem semantics ----
 * Variable 0 is the constant One; spx_cs_new_input returns instance variables (Variable::Instance,
 * numbered before witnesses in z = v || w), spx_cs_new_witness returns witness variables (bit 63
 * set). Linear combinations are compactified on export (sorted, merged, zeros dropped:
 * LinearCombination::compactify / inline_all_lcs). spx_cs_make_square follows test_utils.rs:81-102.
 * spx_cs_matrices exports CSR rows (constraints) over columns z and v / w value bytes, valid until
 * the next change to the system; they feed spx_index and spx_prove directly. Host only. */
typedef struct spx_cs spx_cs;
typedef struct {
    const uint64_t *vars;    /* len variables */
    const uint8_t *coeffs;   /* len canonical Fr, 32 B each */
    size_t len;
} spx_lc;
const char *spx_cs_last_error(void);
int spx_cs_create(spx_cs **out);
int spx_cs_free(spx_cs *cs);
int spx_cs_new_input(spx_cs *cs, const uint8_t value[32], uint64_t *var);
int spx_cs_new_witness(spx_cs *cs, const uint8_t value[32], uint64_t *var);
int spx_cs_enforce(spx_cs *cs, const spx_lc *a, const spx_lc *b, const spx_lc *c);
int spx_cs_make_square(spx_cs *cs, uint64_t num_formatted_variables);
int spx_cs_counts(const spx_cs *cs, uint64_t *constraints, uint64_t *instance, uint64_t *witness);
int spx_cs_is_satisfied(spx_cs *cs, int *ok);
int spx_cs_matrices(spx_cs *cs, spx_csr *a, spx_csr *b, spx_csr *c, const uint8_t **v, const uint8_t **w);

/* ---- synthetic instances (SURVEY §8(d) generators; SplitMix64, same draws as the test oracle) ----
 * kind 0 = uniform-3n (satisfiable, nnz = 3n), 1 = ref-shaped (TestSynthesizer, param = density),
 * 3 = circuit-3n (fixed index, nnz = 3n, many witnesses: param = witness seed of spx_synth_z).
 * spx_synth_csr fills views into the handle (valid until spx_synth_free). */
typedef struct spx_synth spx_synth;
int spx_synth_create(int kind, int log_n, int log_v, uint64_t seed, uint64_t param, spx_synth **out);
uint64_t spx_synth_nnz(const spx_synth *s, int m);
int spx_synth_csr(const spx_synth *s, int m, spx_csr *out);
const uint8_t *spx_synth_z(const spx_synth *s);
/* kind 3 only: the witnesses (z = v || w, canonical, 32 n bytes each) of seeds wseed0 .. wseed0 + count - 1 */
int spx_synth_witnesses(const spx_synth *s, uint64_t wseed0, int count, uint8_t *z_out);
int spx_synth_free(spx_synth *s);

/* ---- live kernel statistics (HIP events on the library's stream, enabled per ctx) ----
 * ids: see SPX_K_* below; per id: launches, summed device ms, summed algorithmic bytes. */
enum {
    SPX_K_SC1 = 0,      /* sumcheck #1 round (fold + evaluate) */
    SPX_K_SC2 = 1,      /* sumcheck #2 round */
    SPX_K_SPMV = 2,     /* Az, Bz, Cz */
    SPX_K_MTV = 3,      /* sum_m r_m M(r_x, .) */
    SPX_K_OPEN = 4,     /* mKZG quotient / fold level */
    SPX_K_EQ = 5,       /* eq tables */
    SPX_K_MSM_SORT = 6, /* the bucket sort: k_sort_count .. k_sort_final (both curves) */
    SPX_K_ACC_G1 = 7,   /* bucket accumulation, affine level, G1 */
    SPX_K_ACC_G2 = 8,   /* bucket accumulation, affine level, G2 */
    SPX_K_ACCX_G1 = 9,  /* bucket accumulation, XYZZ levels, G1 */
    SPX_K_ACCX_G2 = 10, /* bucket accumulation, XYZZ levels, G2 */
    SPX_K_RED_G1 = 11,  /* bucket weighting + final reduction, G1 */
    SPX_K_RED_G2 = 12,  /* bucket weighting + final reduction, G2 */
    SPX_K_COUNT = 13
};
int spx_kernel_stats_enable(spx_ctx *ctx, int on);
int spx_kernel_stats(spx_ctx *ctx, int id, uint64_t *launches, double *ms, double *bytes);
/* the same, restricted to the launches of `id` with the largest algorithmic bytes (e.g. round 1 of a
 * sumcheck, where the tables stream from HBM) */
int spx_kernel_stats_largest(spx_ctx *ctx, int id, uint64_t *launches, double *ms, double *bytes);
/* unit operations counted for a kernel id: curve additions (upper bound: zero digits included) for
 * SPX_K_ACC_* (mixed) and SPX_K_ACCX_* (XYZZ); 0 for the others */
int spx_kernel_ops(spx_ctx *ctx, int id, double *ops);
/* MSM batches of this context rerun with one key slot per digit because a proof-sharded rank's
 * compacted keys overflowed their planned capacity (scalars crowding one rank's buckets); a
 * diagnostic: the results are exact either way */
int spx_msm_reruns(spx_ctx *ctx, uint64_t *reruns);

/* Scalar skew met by this context's MSMs, cumulative: out[0] MSM batches run, out[1] batches with at
 * least one hot bucket (see spx_ctx_set_msm_hot), out[2] hot buckets reduced, out[3] the largest
 * number of partials the weighting leaf added for one bucket (<= 4 with the reduction on). Read from
 * the status words that come back with each batch's results: no extra synchronisation. A diagnostic:
 * the results are exact either way. */
int spx_msm_skew_stats(spx_ctx *ctx, uint64_t out[4]);

/* The MSM window plan. An MSM of `size` points runs `windows` signed digits of `c` bits per scalar:
 * c = 17 with 15 windows from 2^SPX_MSM_WIDE_MIN_LOG points on (environment, default 18; 0: never;
 * otherwise at least 8; read when a public parameter is loaded or generated and at spx_msm_g1 / _g2),
 * c = 16 with 16 windows for the other MSMs of >= 2^14 points, narrower windows below.
 * spx_msm_window_plan: the plan spx_msm_g1 / _g2 would take now (no GPU needed).
 * spx_pp_window_plan: the plan fixed in a public parameter, level = -1 for the commitment bases,
 * 0 .. nv - 1 for the opening levels (2^(nv - level - 1) points); a level at or above the threshold
 * keeps c = 16 where 2^16 buckets more would pass an opening batch's bucket limit (2^19). */
int spx_msm_window_plan(uint64_t size, int *c, int *windows);
/* c[0 .. nv - 1]: the window bits a public parameter of nv variables (1 .. 26) would fix for its
 * opening levels now (no GPU needed) */
int spx_msm_level_plan(int nv, int *c);
int spx_pp_window_plan(spx_pp *pp, int level, int *c, int *windows);

/* ---- kernel-level entry points (parity tests) ---- */
int spx_sum_over_y(spx_ctx *ctx, const spx_csr *m, const uint8_t *z, uint8_t *out);
int spx_eval_on_x(spx_ctx *ctx, const spx_csr *m, const uint8_t *r_x, uint8_t *out);
/* one AHPForMLSumcheck::prove_round [linear-sumcheck] of sum_b f(b) g(b) over n = 2^k canonical Fr
 * (the second sumcheck's product shape, prover.rs:239-247): r_prev = NULL is the first round; with
 * r_prev both tables are first bound at variable 0 to it (f_out / g_out receive the n / 2 bound
 * entries, either may be NULL) and the round runs on the bound tables. evals_out = P(0), P(1), P(2). */
int spx_sumcheck_round(spx_ctx *ctx, const uint8_t *f, const uint8_t *g, size_t n, const uint8_t *r_prev,
                       uint8_t *evals_out, uint8_t *f_out, uint8_t *g_out);
int spx_msm_g1(spx_ctx *ctx, const uint8_t *bases, const uint8_t *scalars, size_t n, uint8_t *out96);
int spx_msm_g2(spx_ctx *ctx, const uint8_t *bases, const uint8_t *scalars, size_t n, uint8_t *out192);
/* the batch verifier's kernels. Decompression of n ark-serialize compressed points (48 / 96 B each) to
 * uncompressed ones (96 / 192 B): ok[j] = 1 for an accepted point (infinity carries the ark flag), 0 for
 * a non-canonical x or an x with no point on the curve (its output bytes are zero). */
int spx_g1_decompress(spx_ctx *ctx, const uint8_t *in, size_t n, uint8_t *out_uncompressed, uint8_t *ok);
int spx_g2_decompress(spx_ctx *ctx, const uint8_t *in, size_t n, uint8_t *out_uncompressed, uint8_t *ok);
/* the compressed public-parameter loader's and serializer's kernels. _decompress_bulk: the contract of
 * spx_g1_decompress / spx_g2_decompress through the loader's throughput kernels. _compress: n uncompressed
 * points (canonical; infinity by the ark flag) to 48 / 96 compressed bytes each. After any of these six
 * calls the first entry of spx_last_timings is the device time of the conversion kernel alone. */
int spx_g1_decompress_bulk(spx_ctx *ctx, const uint8_t *in, size_t n, uint8_t *out_uncompressed, uint8_t *ok);
int spx_g2_decompress_bulk(spx_ctx *ctx, const uint8_t *in, size_t n, uint8_t *out_uncompressed, uint8_t *ok);
int spx_g1_compress(spx_ctx *ctx, const uint8_t *in_uncompressed, size_t n, uint8_t *out_compressed);
int spx_g2_compress(spx_ctx *ctx, const uint8_t *in_uncompressed, size_t n, uint8_t *out_compressed);
/* out[s] = sum_{seg_off[s] <= i < seg_off[s + 1]} scalar_i base_i for n uncompressed bases and n canonical
 * Fr scalars; seg_off: nseg + 1 ascending offsets from 0 to n. Infinity carries the ark flag in both
 * directions. */
int spx_lincomb_g1(spx_ctx *ctx, const uint8_t *bases_uncompressed, const uint8_t *scalars, size_t n,
                   const uint64_t *seg_off, size_t nseg, uint8_t *out_uncompressed);
int spx_lincomb_g2(spx_ctx *ctx, const uint8_t *bases_uncompressed, const uint8_t *scalars, size_t n,
                   const uint64_t *seg_off, size_t nseg, uint8_t *out_uncompressed);
/* ---- subgroup membership ("Subgroup membership") ----
 * Membership of the prime-order subgroups G1 / G2 by the fixed-scalar endomorphism tests (phi(P) = -[z^2] P
 * on G1, psi(P) = [z] P on G2), which is what arkworks' checked deserialization adds to the canonical-
 * encoding and on-curve checks that every entry point of this library makes. Everything here is opt-in:
 * with nothing set, spx_pp_load, spx_verify and spx_verify_many behave as before.
 *
 * spx_g1_in_subgroup / spx_g2_in_subgroup: n uncompressed points (96 / 192 B each) tested on the ctx's
 * GPU. ok[j] = 1 for a member (infinity included), 0 for a non-member, a non-canonical coordinate or a
 * point off the curve. */
int spx_g1_in_subgroup(spx_ctx *ctx, const uint8_t *pts_uncompressed, size_t n, uint8_t *ok);
int spx_g2_in_subgroup(spx_ctx *ctx, const uint8_t *pts_uncompressed, size_t n, uint8_t *ok);
/* the same test of one point (curve 1: G1, 96 B; 2: G2, 192 B) on the host; no GPU. A caller can check
 * the points of a verifier parameter with it: spx_verify / spx_verify_many trust vp and never check it. */
int spx_point_in_subgroup_host(int curve /* 1 | 2 */, const uint8_t *pt_uncompressed, int *ok);
/* Checks every raw G1 and G2 level of a loaded or generated public parameter on the ctx's GPU, and g and
 * h on the host (spx_pp_load itself does not: the check is load time a trusted file does not need).
 * SPX_OK with *bad = 0, or SPX_SERIALIZATION with *bad = the number of points outside their subgroup and
 * spx_last_error naming the first one. first = {curve (1 | 2), level (UINT64_MAX for g / h), index} of
 * the lowest offender in the order G1 levels, G2 levels, g, h: the same whatever order the GPU ran in.
 * bad and first may each be NULL. Every rank of a sharded context holds the complete raw levels, so the
 * call works on any context of the public parameter's device. */
int spx_pp_check_subgroup(spx_ctx *ctx, spx_pp *pp, uint64_t *bad, uint64_t first[3]);

/* ---- public-parameter structure, derived verifier parameter, views ("Public-parameter
 * structure and views") ----
 * With bit 0 of x paired with t_i, the levels of a well-formed parameter satisfy
 *   powers_of_g[i][2b] + powers_of_g[i][2b+1] = powers_of_g[i+1][b]   (the last level's pair sums to g),
 *   sum_b powers_of_g[i][2b+1] = g^{t_i} = vp.g_mask_random[i],
 * the same for powers_of_h and h, and the parameter of nv' < nv variables is levels nv - nv' .. nv - 1. */

/* MLPolyCommit::verify (commitment/verify.rs:12-45). Host only, no GPU. com56 = spx_commit's output,
 * proof = spx_open's proof_out (96 + 8 + 96 nv bytes), point = nv canonical Fr. *accepted = 1 | 0.
 * Malformed bytes: SPX_SERIALIZATION; nv != vp.nv or a wrong length: SPX_INVALID_ARGUMENT. */
int spx_pc_verify(const uint8_t *vp, size_t vp_len, const uint8_t com56[56], const uint8_t *point, int nv,
                  const uint8_t value[32], const uint8_t *proof, size_t proof_len, int *accepted);

/* VerifierParameter of ANY public parameter (loaded, generated, or a view), uncompressed, in
 * spx_vp_from_pp's format: g_mask_random[i] = sum of the odd-index points of powers_of_g[i], summed on
 * the ctx's GPU. For a generated parameter the bytes equal spx_vp_from_pp's. The call does not run the
 * structure check: the result is meaningful for a parameter that passes spx_pp_check_structure. */
int spx_pp_derive_vp(spx_ctx *ctx, spx_pp *pp, uint8_t *out, size_t cap, size_t *len);

/* Structure of a public parameter, in two stages, on the ctx's GPU.
 * Stage 1 (exact): the fold relation for every pair of every level of both curves.
 *   *bad = number of failing pairs.
 *   first = {curve 1 | 2, level, pair index b} of the lowest failing pair, in the order G1 levels, G2
 *   levels, by level, then b (pair b of level i is points 2b, 2b+1 against point b of level i+1; the
 *   last level's only pair is against g / h).
 * Stage 2 (only if stage 1 passed; otherwise *opening_ok = -1): a commitment to a pseudo-random table,
 *   opened at a pseudo-random point, must verify (spx_pc_verify's equation) under the derived VP.
 *   *opening_ok = 1 | 0.
 * entropy32 seeds stage 2's table and point. With NULL a fixed seed is used: that finds damage, not an
 * adversary who knows the seed.
 * Returns SPX_OK, or SPX_SERIALIZATION with spx_last_error naming the pair ("powers_of_h level 3 pair 17:
 * points 34 + 35 != level 4 point 17 (2 such pairs)") or "opening self-test failed".
 * bad, first and opening_ok may each be NULL. Afterwards spx_last_timings holds the two stages' wall
 * time and the device time of stage 1's two kernels, in microseconds. */
int spx_pp_check_structure(spx_ctx *ctx, spx_pp *pp, const uint8_t *entropy32, uint64_t *bad,
                           uint64_t first[3], int *opening_ok);

/* The public parameter of nv variables (1 <= nv <= parent's) that a larger one contains: levels
 * parent_nv - nv .. parent_nv - 1 of both curves, and g, h. The handle behaves as a PP of nv variables in
 * every call that takes an spx_pp. It borrows the parent's device storage (the raw levels and the G2
 * opening tables, with the parent's window bits; spx_pp_window_plan reports them) and builds only its own
 * G1 commitment table; with nv == the parent's it shares that too. Ownership of the storage is shared: the
 * parent may be freed first. A view of a view refers to the root's storage. ctx must be on the parent's
 * device (SPX_INVALID_ARGUMENT otherwise, as for nv out of range or a NULL handle). */
int spx_pp_view(spx_ctx *ctx, spx_pp *parent, int nv, spx_pp **out);

/* out[0] device bytes this handle allocated itself, out[1] device bytes it borrows from a parent (0 for a
 * loaded / generated PP), out[2] handles alive on the storage it uses (itself included). No GPU call. */
int spx_pp_mem_info(spx_pp *pp, uint64_t out[3]);
/* Subgroup check of proof points in spx_verify and spx_verify_many on this context: 0 = off (the
 * default: every status and message as before), 1 = on, -1 = the process default (SPX_SUBGROUP_CHECK=1
 * -> on, else off). On: spx_verify tests the commitment and every point of the two opening proofs right
 * after decompressing it, before any transcript replay or algebraic check, and a non-member fails with
 * SPX_SERIALIZATION and a message naming the field ("commitment", "opening 1 h", "opening 2 proof point
 * 3": "... is not in the prime-order subgroup"), as Proof::deserialize does in the reference
 * (/root/reference/src/benchmark.rs:45). spx_verify_many tests a batch's points on the GPU behind their
 * decompression; a proof with a rejected point goes to the single-proof path, and status[j] is still what
 * spx_verify gives for proof j on a context with the same setting. vp is not checked.
 * SPX_INVALID_ARGUMENT while the context is in use. */
int spx_ctx_set_subgroup_check(spx_ctx *ctx, int mode);
/* membership checks made through this context, cumulative: out[0] points checked on the GPU, out[1] points
 * checked on the host, out[2] points rejected as reported to the caller (ok = 0, a public parameter's
 * offenders, a strict spx_verify's error; a batch's rejected point counts once, on the single-proof path) */
int spx_subgroup_stats(spx_ctx *ctx, uint64_t out[3]);
/* ---- witness check: reject a witness with (Az)o(Bz) != Cz on the GPU before proving it.
 * The check is of the tables the proof is built from: Az, Bz, Cz as the prover's sum_over_y computes them
 * (r1cs_reader.rs:75-85). For a matrix row that names a column more than once the last entry wins, as in
 * the proof, not ark-relations' sum of the entries.
 * 0 = off (the default: every call behaves as before), 1 = on, -1 = process default (SPX_WITNESS_CHECK=1 -> on).
 * SPX_INVALID_ARGUMENT while the context is in use. Every rank of a proof-sharded prove must use the same
 * mode (ranks that differ fail their next sharded prove with SPX_INVALID_ARGUMENT).
 * On: spx_prove, spx_prove_witness and spx_prover_first_round return SPX_WRONG_WITNESS for a witness that
 * violates a constraint, with "constraint 37 is not satisfied: (Az)(Bz) != Cz (5 of 256 constraints fail)"
 * in spx_last_error (the lowest violated row); no proof byte is written and *len is left untouched. The
 * check is one kernel behind the prover's first one and is read at the proof's first host wait.
 * spx_prove_many sets lens[i] = 0 for a rejected witness, goes on to that worker's next proof, produces
 * every other proof and returns SPX_WRONG_WITNESS, spx_last_error naming the lowest rejected proof index
 * and its row ("proof 2: constraint ..."); any other failure stops its worker and is returned as before.
 * spx_witness_check on a rejected witness gives its row. */
int spx_ctx_set_witness_check(spx_ctx *ctx, int mode);
/* SPX_OK with *bad = 0, or SPX_WRONG_WITNESS with *bad = number of violated constraints, *first_row = the
 * lowest one, abc = Az, Bz, Cz of that row as canonical Fr (96 B). bad, first_row, abc may each be NULL.
 * (*first_row = UINT64_MAX and abc = 0 when nothing is violated.) Runs whatever the context's mode is; on
 * a proof-sharded context every rank must call it, and every rank gets the same answer. */
int spx_witness_check(spx_ctx *ctx, spx_pk *idx, spx_witness *wit, uint64_t *bad, uint64_t *first_row, uint8_t *abc);
/* cumulative, this context: out[0] witnesses checked, out[1] witnesses rejected, out[2] check kernel
 * launches (a lockstep group's checks are one), out[3] rows checked. All stay put while the check is off. */
int spx_witness_check_stats(spx_ctx *ctx, uint64_t out[4]);
int spx_commit(spx_ctx *ctx, spx_pp *pp, const uint8_t *table, int nv, uint8_t *out56);
/* proof_out: Proof{h, proofs} compressed = 96 + 8 + 96 * nv bytes */
int spx_open(spx_ctx *ctx, spx_pp *pp, const uint8_t *table, int nv, const uint8_t *point, uint8_t *eval_out,
             uint8_t *proof_out);

#ifdef __cplusplus
}
#endif
#endif
