/*
 * bdls_hip.h -- C ABI of libbdlship.so, the MI355X (gfx950) batched ECDSA
 * verification engine for the BDLS / Fabric signature-verification hot path.
 *
 * Drop-in boundary: the reference verifies every signature through the BCCSP
 * provider interface, one call at a time:
 *   bccsp/bccsp.go:125             BCCSP.Verify(k Key, signature, digest []byte, opts) (bool, error)
 *   bccsp/sw/impl.go:247-270       sw CSP.Verify (arg checks + verifier dispatch)
 *   bccsp/sw/ecdsa.go:41-57        verifyECDSA (DER unmarshal, low-S, crypto/ecdsa.Verify)
 *   bccsp/sw/hash.go:29-33         hasher.Hash (SHA-256)
 *   msp/identities.go:170-199      identity.Verify = Hash(msg) + Verify(pk, sig, digest)
 * The entry points below are what a `bccsp/hip` provider binds over cgo (see
 * INTEGRATION.md): plain pointers and sizes, no Go or torch types.
 *
 * Result encoding for every verify entry point:
 *   bitmap : ceil(n/8) bytes (host API) or ceil(n/64) uint64 words (device
 *            API), LSB-first: bit i set <=> record i verified (Go returns true).
 *   reason : n bytes, BH_R_* below. Codes 1..6 correspond to Go returning
 *            (false, err) from BCCSP.Verify; 7..10 to (false, nil).
 * Function return: BH_OK (0) or a negative BH_E_* (then bh_last_error()).
 * Thread-safety: all entry points may be called concurrently from several
 * host threads; calls on one device are serialized internally.
 */
#ifndef BDLS_HIP_H
#define BDLS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- return codes ---- */
#define BH_OK 0
#define BH_E_INVALID (-1) /* bad argument */
#define BH_E_NOT_INIT (-2) /* bh_init not called / device not initialised */
#define BH_E_DEVICE (-3)   /* HIP runtime error */
#define BH_E_NODEV (-4)    /* no usable gfx950 device */
#define BH_E_NOMEM (-5)    /* device allocation failed */

/* ---- per-record reason codes (bit 0 of the bitmap is 1 iff BH_R_OK) ---- */
#define BH_R_OK 0
#define BH_R_EMPTY_SIG 1    /* impl.go:252  "Invalid signature. Cannot be empty."      -> error */
#define BH_R_EMPTY_DIGEST 2 /* impl.go:255  "Invalid digest. Cannot be empty."         -> error */
#define BH_R_DER 3          /* utils/ecdsa.go:44 asn1.Unmarshal failed                  -> error */
#define BH_R_R_NONPOS 4     /* utils/ecdsa.go:57 "R must be larger than zero"           -> error */
#define BH_R_S_NONPOS 5     /* utils/ecdsa.go:60 "S must be larger than zero"           -> error */
#define BH_R_HIGH_S 6       /* sw/ecdsa.go:53 "Invalid S. Must be smaller than half..." -> error */
#define BH_R_BAD_KEY 7      /* ecdsa.Verify: Q not a valid curve point                  -> false */
#define BH_R_R_RANGE 8      /* ecdsa.Verify: r >= n                                     -> false */
#define BH_R_MATH 9         /* ecdsa.Verify: x(u1 G + u2 Q) mod n != r, or infinity    -> false */
#define BH_R_S_RANGE 10     /* ecdsa.Verify: s >= n (only with BH_F_NO_LOW_S)           -> false */
#define BH_R_UNSUPPORTED 11 /* bh_verify_x509: not an ecdsa-with-SHA256 P-256 certificate
                               signature this engine checks (the caller uses Go's x509);
                               bh_verify_x509_ex: not ecdsa-with-SHA256 / -SHA384 / -SHA512 */

/* ---- flags ---- */
#define BH_F_HASH_SHA256 1u /* msg[i] is a message; digest = SHA-256(msg[i]) (identity.Verify) */
#define BH_F_NO_LOW_S 2u    /* do not apply Fabric's low-S rule (plain crypto/ecdsa.Verify) */
#define BH_F_KEEP_KEYS 4u   /* keys used >= 2 times in the batch get a table in the device's
                               key registry (kept across calls, see bh_keys_register) */
#define BH_F_HASH_SHA3_256 8u /* msg[i] is a message; digest = SHA3-256(msg[i]): identity.Verify
                                 of an MSP with SignatureHashFamily SHA3 (msp/identities.go:
                                 219-227, bccsp/sw/new.go:72). Exclusive with BH_F_HASH_SHA256. */
#define BH_F_ANY_LANE 16u   /* bh_verify_dev on the library's streams (stream NULL, no timing):
                               consecutive calls rotate over the device's compute lanes
                               (BH_LANES, default 3, at most 4), each with its own workspace,
                               so a pass runs beside the previous calls' passes as host
                               batches do. The k-th BH_F_ANY_LANE pass of a device is
                               ordered after the (k-4)-th (whatever lane each took and
                               whatever other work ran between them), so a caller that
                               rotates 4 output sets never has two in-flight passes
                               writing one set; bh_sync waits for every lane.
                               Ignored elsewhere (host batches already alternate lanes). */
#define BH_F_HASH_SHA384 32u /* msg[i] is a message; digest = SHA-384(msg[i]): the hash of the
                                sw provider's security level 384 (bccsp/sw/conf.go:43-46,
                                bccsp/sw/new.go:69-73, SHA384Opts) and of ecdsa-with-SHA384
                                certificates. */
#define BH_F_HASH_SHA512 64u /* msg[i] is a message; digest = SHA-512(msg[i]) (ecdsa-with-SHA512
                                certificates).
                                Both are taken by bh_verify and bh_verify_dev only, for
                                BH_CURVE_P256 and BH_CURVE_P384, with the semantics of
                                BH_F_HASH_SHA256 (length 0 hashes the empty message, an empty
                                signature is BH_R_EMPTY_SIG, low-S unless BH_F_NO_LOW_S; reasons,
                                precedence and bitmap unchanged); e = hashToNat of the digest:
                                its leftmost 32 bytes (P-256) or 48 (P-384), reduced mod n. The
                                four BH_F_HASH_* flags are mutually exclusive. A digest pass
                                hashes every record of a chunk into library workspace (not part
                                of bh_workspace_bytes; allocated per device at first use) and
                                the curve's pass then runs in digest mode. With either flag,
                                BH_F_ANY_LANE and BH_F_KEEP_KEYS are ignored, and a P-256
                                batch runs the way a P-384 batch does: behind every lane's
                                work, and bh_verify on the first initialised device alone in
                                chunks of BH_P384_CHUNK records (bh_verify_dev hashes a
                                resident P-256 batch in one pass). bh_timing.prep_ms includes
                                the digest pass; bh_device_stats counts one batch per call.
                                Every other entry point answers BH_E_INVALID for them. */
#define BH_F_BATCH_KEYS 128u /* BH_CURVE_P384 passes: a key that at least 4 records of one pass
                                (one chunk of BH_P384_CHUNK records) use, counting only the
                                records that pass the checks before the curve arithmetic, gets
                                a comb table for that pass -- 6 teeth x 64 bits, 63 affine
                                entries, 7,056 bytes, built in library workspace and gone with
                                the pass; nothing is registered or kept. Each record takes the
                                first route that applies: its key is in the bh_keys384_*
                                registry -> the registry's table route, as without the flag;
                                its key has a comb -> the comb route (64 doublings with u1 G
                                folded in from a comb of G, about 1,900 field products against
                                the ladder's 5,600); otherwise the ladder, which also reports
                                the reason of every record the checks rejected. Results never
                                depend on the flag: bitmap and reasons are bit for bit those of
                                the unflagged call, in bh_verify, bh_verify_dev and
                                bh_verify_mixed's P-384 group, with every BH_F_HASH_* flag,
                                two-span messages and BH_F_NO_LOW_S. Accepted by every entry
                                point and ignored wherever the pass is not P-384 (a P-256 pass
                                finds its repeated keys unasked). The comb of G, the grouping
                                tables and the comb slots (one per 4 records of a chunk, about
                                3.8 KB per record of the largest chunk) are allocated at a
                                device's first flagged pass and freed by bh_shutdown; callers
                                that never set the flag pay nothing.
                                bh_timing of a flagged bh_verify_dev call, per chunk and
                                summed: prep_ms and inv_ms as ever; plan_ms from the end of
                                the inverse to the end of grouping and routing; then two
                                streams run side by side from that point: the ladder route,
                                and the comb build followed by the table routes (comb, then
                                registry). build_ladder_ms = (routing end -> comb build end) +
                                (routing end -> ladder end); keycomb_ms = comb build end ->
                                end of both table routes; the two overlap in time, so they do
                                not add up to the pass. n_keytables = combs built, n_keycomb =
                                records on either table route, n_ladder = the rest.
                                When to set it (65,536 resident records): 1.17 x
                                at 16 and at 1,024 uses per key, 0.995 x on all-distinct keys,
                                0.73 x at exactly 4 uses per key (the comb build, one lane per
                                key, dominates there): set it for batches with a dozen or more
                                records per key. BH_P384_COMB_MIN (2 .. 65535, read once) replaces the 4
                                for experiments. */

#define BH_CURVE_P256 0
#define BH_CURVE_SECP256K1 1
#define BH_CURVE_P384 2 /* the sw provider's second NIST curve (bccsp/sw/conf.go:59-61,
                           security level 384). Taken by bh_verify and bh_verify_dev only, with
                           the semantics they have for P-256 (Go-asn1 DER, R, S > 0, low-S with
                           P-384's half order, pointFromAffine, r, s < n, hashToNat, the x
                           check) and the same BH_R_* codes, precedence and bitmap. Keys are
                           96 bytes (X || Y, 48 each). BH_F_HASH_SHA256 / BH_F_HASH_SHA3_256 as
                           for P-256 (identity.Verify hashes with the MSP's family whatever the
                           key's curve, msp/identities.go:170-227); in digest mode any length
                           >= 1: the leftmost 48 bytes, a shorter digest whole, one reduction
                           mod n. BH_F_KEEP_KEYS and BH_F_ANY_LANE are ignored; BH_F_BATCH_KEYS
                           gives keys repeated within a pass a comb for that pass. Every other
                           entry point with a curve argument answers BH_E_INVALID for this curve;
                           the compact and the staged BatchVerify for it are entry points of
                           their own (bh_verify384_compact, bh_batch_verify384_ptrs). */

/* Bytes of one public key (X || Y) in bh_batch.pub for a curve: 64, 64, 96;
 * negative for an unknown curve. */
int bh_curve_key_bytes(int curve);

/* One batch of verify records (structure of arrays). Host pointers for
 * bh_verify(), device pointers for bh_verify_dev(). */
typedef struct bh_batch {
  const uint8_t *pub;      /* n * 64 bytes: Q.x || Q.y, 32-byte big-endian each (P-384:
                              n * 96, 48-byte coordinates; bh_curve_key_bytes)           */
  const uint8_t *sig;      /* concatenated ASN.1 DER signatures                          */
  const uint64_t *sig_off; /* n byte offsets into sig                                    */
  const uint32_t *sig_len; /* n lengths (0 -> BH_R_EMPTY_SIG)                            */
  const uint8_t *msg;      /* concatenated messages (BH_F_HASH_SHA256) or digests        */
  const uint64_t *msg_off; /* n byte offsets into msg                                    */
  const uint32_t *msg_len; /* n lengths (digest mode: 0 -> BH_R_EMPTY_DIGEST)            */
} bh_batch;

/* The same records in the COMPACT host layout (round 4; VERDICT r3: the host
 * path sat at its PCIe bound with 24 B of u64 offsets + u32 lengths per
 * record and a 64-byte key copy per record). A Go BatchVerify holds bccsp.Key
 * objects, many of them the same identity's key (the MSP identity cache), so
 * the binding passes each distinct key once and a u32 index per record;
 * offsets are the prefix sums of the lengths (the device computes them), and
 * a batch of equal-length messages (digests, fixed-size payloads) sends no
 * lengths at all. 339 B per config-2 record instead of 424. Verification is
 * bit-for-bit that of the expanded bh_batch, record i having key keys[key_idx[i]],
 * signature and message the i-th spans of sig / msg. Host pointers. */
typedef struct bh_cbatch {
  const uint8_t *keys;      /* nkeys * 64: distinct public keys X || Y            */
  const uint32_t *key_idx;  /* n: record i's key index (< nkeys); NULL: keys holds
                               one key per record, in record order (nkeys = n)   */
  size_t nkeys;
  const uint8_t *sig;       /* concatenated DER signatures, record order         */
  const uint32_t *sig_len;  /* n lengths; record i's offset = sum of the earlier  */
  const uint8_t *msg;       /* concatenated messages (BH_F_HASH_*) or digests     */
  const uint32_t *msg_len;  /* n lengths, or NULL: every message is msg_stride B  */
  uint32_t msg_stride;
} bh_cbatch;

/* Per-call stage timing (milliseconds, HIP events on the launch stream) and
 * routing counts. */
typedef struct bh_timing {
  float prep_ms;       /* parse + checks + SHA-256 / BLAKE2b + Montgomery inputs */
  float inv_ms;        /* batched s^-1 mod n, u1, u2 */
  float plan_ms;       /* registry lookup + public-key dedup + routing */
  float build_ladder_ms; /* one grid: per-key fixed-base table builds and the
                            variable-base ladder for records without a table */
  float publish_ms;    /* registry publication of new tables (BH_F_KEEP_KEYS) */
  float keycomb_ms;    /* u2 Q from key tables + u1 G + x check, bitmap */
  uint32_t n_keycomb;  /* records verified on the key-table path */
  uint32_t n_ladder;   /* records verified on the ladder path */
  uint32_t n_keytables; /* tables built in this call */
  uint32_t wide;       /* lanes per record on the key-table path */
} bh_timing;

/* Initialise the devices in device_mask (bit d = HIP device d; 0 = all
 * visible). Builds the per-device fixed-base tables. Idempotent. */
int bh_init(uint32_t device_mask, uint32_t flags);
int bh_shutdown(void);
int bh_device_count(void);          /* devices initialised by bh_init */
const char *bh_last_error(void);    /* thread-local message for the last failure */
const char *bh_version(void);

/* Device-memory bytes of library workspace needed per device for n records. */
size_t bh_workspace_bytes(size_t n);

/* Host-memory batch: copies to the devices, shards [0,n) over all initialised
 * devices (contiguous ranges, no collective), gathers bitmap and reasons.
 * curve: BH_CURVE_P256 (the Fabric/BCCSP path; secp256k1 BDLS messages use
 * bh_verify_bdls) or BH_CURVE_P384. A P-384 batch runs on the first
 * initialised device alone, uploaded, verified and downloaded in chunks of
 * BH_P384_CHUNK records (environment, read once, rounded up to 64; default
 * 65536); the device's P-384 workspace and fixed-base table of G are made at
 * its first P-384 call (bh_init's cost does not change). bh_device_stats
 * counts such a call as one batch, however many chunks it runs in. */
int bh_verify(int curve, const bh_batch *b, size_t n, uint32_t flags, uint8_t *bitmap,
              uint8_t *reason);

/* bh_verify with two-span messages: record i's signed bytes are
 * msg[msg_off[i], +msg_len[i]) || msg[msg2_off[i], +msg2_len[i]) (msg2_len 0 =
 * one span), hashed on the device (BH_F_HASH_SHA256 or BH_F_HASH_SHA3_256
 * required). Replaces the host-side concatenation of a Fabric endorsement's
 * SignedData, Data = prp || endorser (core/common/validation/statebased/
 * validator_keylevel.go:246-260; core/committer/txvalidator/v20/plugindispatcher),
 * so both spans can point into the serialized block itself. */
int bh_verify_2seg(int curve, const bh_batch *b, const uint64_t *msg2_off,
                   const uint32_t *msg2_len, size_t n, uint32_t flags, uint8_t *bitmap,
                   uint8_t *reason);

/* A host-memory batch whose records may be of either NIST curve (a Fabric
 * channel where one org's CA issues P-384 certificates: bccsp/sw/keyimport.go
 * imports any *ecdsa.PublicKey, and identity.Verify hashes with the MSP's
 * 256-bit family whatever the key's curve, msp/identities.go:170-227).
 * Record i is verified under curve[i]; its key is the bh_curve_key_bytes(curve[i])
 * bytes at pub + pub_off[i]; its message is msg[msg_off[i], +msg_len[i]) ||
 * msg[msg2_off[i], +msg2_len[i]) (msg2_off and msg2_len both NULL, or
 * msg2_len[i] = 0: one span; second spans need a fused hash flag).
 * The result for record i is, bit for bit, what bh_verify gives that record
 * alone under curve[i] with the same flags (two spans: over the concatenated
 * message). flags: BH_F_HASH_SHA256, BH_F_HASH_SHA3_256, BH_F_NO_LOW_S and
 * BH_F_KEEP_KEYS (the P-256 records; ignored for P-384, whose kept tables are
 * the bh_keys384_* registry's). BH_F_HASH_SHA384 / BH_F_HASH_SHA512 are refused.
 * The P-256 records run as a bh_verify_2seg / bh_verify batch over all
 * devices, the P-384 records as a bh_verify batch on the first device;
 * bh_device_stats counts one batch per non-empty curve group. Every bit of
 * the ceil(n / 8) bitmap bytes is written (padding bits zero). */
typedef struct bh_mbatch {
  const uint8_t  *curve;    /* n: BH_CURVE_P256 or BH_CURVE_P384 per record */
  const uint8_t  *pub;      /* record i's key at pub + pub_off[i] */
  const uint64_t *pub_off;
  const uint8_t  *sig;  const uint64_t *sig_off;  const uint32_t *sig_len;
  const uint8_t  *msg;  const uint64_t *msg_off;  const uint32_t *msg_len;
  const uint64_t *msg2_off; const uint32_t *msg2_len;  /* both NULL: one span */
} bh_mbatch;
int bh_verify_mixed(const bh_mbatch *b, size_t n, uint32_t flags, uint8_t *bitmap,
                    uint8_t *reason);

/* Asynchronous form of bh_verify (the pipelined BatchVerify): enqueues the
 * upload (copy stream), the verify passes and the result download (compute
 * stream) on every device and returns at once with *job. bh_verify_wait(job)
 * blocks until the batch is done, writes bitmap / reason and frees the job;
 * every submitted job must be waited exactly once. The caller's input
 * buffers must stay valid and unchanged until then. With two jobs in flight
 * per device, the next batch's H2D runs under this batch's kernels; this needs
 * page-locked inputs (bh_host_alloc) -- pageable inputs are correct but their
 * upload is staged synchronously by the HIP runtime. bh_verify = submit+wait. */
typedef struct bh_job bh_job;
int bh_verify_submit(int curve, const bh_batch *b, size_t n, uint32_t flags, uint8_t *bitmap,
                     uint8_t *reason, bh_job **job);
int bh_verify_wait(bh_job *job);

/* Page-locked host memory, DMA-able by every device (hipHostMalloc portable).
 * A cgo caller packs its SoA batch straight into it (no further copy). */
int bh_host_alloc(size_t bytes, void **ptr);
int bh_host_free(void *ptr);

/* Device-resident batch on one device: every pointer in *b and the outputs
 * are device pointers on `device`. Enqueued on `stream` (hipStream_t; NULL =
 * the library's stream for that device) and synchronised before return when
 * timing != NULL (then filled) or when sync != 0. bitmap_words: ceil(n/64)
 * uint64 words. BH_CURVE_P384: passes of BH_P384_CHUNK records behind every
 * lane's work; timing fills prep_ms, inv_ms and build_ladder_ms (ladder, u1 G
 * and the x check), n_ladder = n. */
int bh_verify_dev(int device, int curve, const bh_batch *b, size_t n, uint32_t flags,
                  uint64_t *bitmap_words, uint8_t *reason, void *stream, int sync,
                  bh_timing *timing);

/* Single signature with exact BCCSP.Verify semantics (the sw provider's
 * Verify for an ECDSA P-256 public key, bccsp/sw/impl.go:247-270). *valid =
 * 1/0, *reason = BH_R_*; return BH_OK unless the engine itself failed.
 * Concurrent callers are COALESCED (the drop-in Verify is called by up to
 * validatorPoolSize goroutines at once, core/peer/config.go:269-272): each
 * call joins the batch being filled and blocks; a library thread submits that
 * batch as soon as a pipeline slot is free (a lone call goes at once; under
 * load, calls arriving while one batch runs share the next device pass).
 * BH_COALESCE_US (environment, default 0) makes an idle flusher linger that
 * many microseconds for more calls. The caller's buffers are copied before
 * the call blocks. */
int bh_csp_verify_p256(const uint8_t pub[64], const uint8_t *sig, size_t sig_len,
                       const uint8_t *digest, size_t digest_len, int *valid, int *reason);
/* Coalescer counters: out[0] single calls served, out[1] device batches they
 * formed, out[2] largest batch. */
int bh_csp_stats(uint64_t out[3]);

/* bh_verify / bh_verify_submit on a compact batch (see bh_cbatch): same
 * results, flags and curves (BH_CURVE_P256), same pipeline and job handles
 * (collect with bh_verify_wait). Replaces the same reference interfaces as
 * bh_verify: BatchVerify over bccsp/sw/impl.go:247-270 / msp identities.go:
 * 170-199. BH_E_INVALID for a key index >= nkeys or a null required field. */
int bh_verify_compact(int curve, const bh_cbatch *b, size_t n, uint32_t flags, uint8_t *bitmap,
                      uint8_t *reason);
int bh_verify_compact_submit(int curve, const bh_cbatch *b, size_t n, uint32_t flags,
                             uint8_t *bitmap, uint8_t *reason, bh_job **job);

/* ---- Staged BatchVerify (round 6) ------------------------------------------
 * BatchVerify straight from the caller's own (pageable, per-record) buffers:
 * the library packs each shard into page-locked staging it owns and reuses
 * (pipeline slot buffers), on a pool of worker threads -- key de-duplication
 * by a lock-free hash table (each distinct key uploaded once + a u32 index per
 * record, the compact layout), lengths, and the signature and message bytes
 * in one pass per record, in chunks whose H2D copies start while the next
 * chunk is packed (include/../bdls_amd/csrc/pack.h).
 * Replaces the per-call packing a Go BatchVerify did on one goroutine into a
 * fresh bh_host_alloc (INTEGRATION.md 2 packBatch) -- the batch points
 * common/policies/policy.go:363-395 and core/committer/txvalidator/v20/
 * validator.go:193-208 -- and the per-call bh_host_alloc/free. Results,
 * flags, curve (BH_CURVE_P256) and job handles as bh_verify_submit (collect
 * with bh_verify_wait); the caller's buffers must stay valid until the
 * submit call RETURNS (everything is copied by then), not until the wait.
 * Worker threads: BH_PACK_THREADS, default the CPUs the process may use
 * (affinity, cgroup quota) less one, at most 15. */
int bh_batch_verify(int curve, const bh_batch *b, size_t n, uint32_t flags, uint8_t *bitmap,
                    uint8_t *reason);
int bh_batch_verify_submit(int curve, const bh_batch *b, size_t n, uint32_t flags,
                           uint8_t *bitmap, uint8_t *reason, bh_job **job);
/* The same records as separate caller buffers -- the form a cgo binding
 * hands over without flattening in Go (pointers pinned with runtime.Pinner,
 * Go >= 1.21): per record its 64-byte key X || Y, its DER signature and its
 * message (BH_F_HASH_*) or digest. A NULL signature / message pointer is a
 * zero-length field (Go's nil slice: BH_R_EMPTY_SIG / BH_R_EMPTY_DIGEST or the
 * hash of the empty message); a NULL key pointer reads as the all-zero point
 * (BH_R_BAD_KEY). Records sharing a key may pass the same pointer or equal
 * bytes: the library de-duplicates by content. */
typedef struct bh_pbatch {
  const uint8_t *const *pub;  /* n pointers to 64 bytes Q.x || Q.y                 */
  const uint8_t *const *sig;  /* n pointers to DER signatures                     */
  const uint32_t *sig_len;
  const uint8_t *const *msg;  /* n pointers to messages (BH_F_HASH_*) or digests  */
  const uint32_t *msg_len;
} bh_pbatch;
int bh_batch_verify_ptrs(int curve, const bh_pbatch *b, size_t n, uint32_t flags,
                         uint8_t *bitmap, uint8_t *reason);
int bh_batch_verify_ptrs_submit(int curve, const bh_pbatch *b, size_t n, uint32_t flags,
                                uint8_t *bitmap, uint8_t *reason, bh_job **job);
/* The last staged shard's packing: out[0] plan ms (lengths -> byte offsets),
 * [1] fill ms (lengths, keys + indices, bytes; the chunks' H2D copies queued
 * as they complete), [2] worker threads,
 * [3] chunks, [4] keys de-duplicated (1/0), [5] keys uploaded, [6] records,
 * [7] the sample's distinct-key estimate (0: no repeat seen), [8] table
 * rebuilds, [9] staged shards since start. Not in the reference
 * (operations metrics). */
int bh_pack_stats(double out[10]);

/* ---- P-384 BatchVerify: compact keys, job handles, every device ---------------
 * The compact and the staged BatchVerify for ECDSA P-384 keys. Replaces
 * BatchVerify over bccsp/sw/impl.go:247-270 and bccsp/sw/ecdsa.go:41-57 for
 * P-384 keys, and the batch points in common/policies/policy.go:363-395, as
 * bh_verify_compact and bh_batch_verify_ptrs do for P-256 (which keep refusing
 * BH_CURVE_P384: these entry points are P-384's own).
 * Results are, bit for bit, those of bh_verify(BH_CURVE_P384) on the expanded
 * batch. Flags: BH_F_HASH_SHA256, BH_F_HASH_SHA3_256, BH_F_NO_LOW_S and
 * BH_F_BATCH_KEYS; BH_F_KEEP_KEYS and BH_F_ANY_LANE are ignored, as everywhere
 * for this curve; BH_F_HASH_SHA384 / BH_F_HASH_SHA512 are refused (BH_E_INVALID:
 * use bh_verify). BH_E_INVALID also for a key index >= nkeys, a null required
 * field and n > 2^32 - 1; BH_E_NOT_INIT before bh_init (argument checks come
 * first). n = 0 is BH_OK; a submit form still returns a job to wait.
 * The batch is dealt over all initialised devices in 64-aligned shards
 * (BH_HOST_SHARDS per device, read once); a device runs a shard in passes of
 * BH_P384_CHUNK records. Each device has two pipeline slots: a shard is copied
 * into page-locked staging the library reuses, uploaded on the copy stream and
 * verified behind the device's earlier P-384 work, so one job's upload runs
 * under another's kernels and the submit forms return once everything is
 * enqueued (a call waits only for a slot that still holds an uncollected shard,
 * or where a buffer has to grow). Jobs are collected with bh_verify_wait,
 * exactly once each, in any order, P-256 jobs among them. bh_device_stats
 * counts one batch per call, however many shards and chunks.
 * Keys are imported (range and curve checks, Montgomery form) and looked up in
 * the bh_keys384_* registry once per distinct key of a shard, not once per
 * record. With BH_F_BATCH_KEYS a pass counts its records per key INDEX (keys of
 * >= BH_P384_COMB_MIN records, default 4, get a comb for that pass): two
 * indices whose 96 bytes happen to be equal count as two keys. Results never
 * depend on that. key_idx = NULL selects the per-record key layout and the
 * grouping by key bytes bh_verify uses.
 *
 * bh_verify384_compact: bh_cbatch as documented with keys of 96 bytes (X || Y,
 * 48 each), keys = nkeys * 96. A shard uploads only the keys its records use.
 * The inputs are copied when the submit call returns. */
int bh_verify384_compact(const bh_cbatch *b, size_t n, uint32_t flags, uint8_t *bitmap,
                         uint8_t *reason);
int bh_verify384_compact_submit(const bh_cbatch *b, size_t n, uint32_t flags, uint8_t *bitmap,
                                uint8_t *reason, bh_job **job);
/* The staged form from the caller's own per-record buffers: bh_pbatch with
 * 96-byte keys. The library de-duplicates keys by content (pack.h at key
 * width 96) and packs into the slot's page-locked staging; NULL sig / msg /
 * key pointers mean what they mean for bh_batch_verify_ptrs. The caller's
 * buffers may be released when the submit call returns. */
int bh_batch_verify384_ptrs(const bh_pbatch *b, size_t n, uint32_t flags, uint8_t *bitmap,
                            uint8_t *reason);
int bh_batch_verify384_ptrs_submit(const bh_pbatch *b, size_t n, uint32_t flags, uint8_t *bitmap,
                                   uint8_t *reason, bh_job **job);

/* Device batches since bh_init over every entry point: out[0] batches launched
 * (one per device pass sequence of a call or shard, one per latency-path
 * batch), out[1] records they carried. Lets a consumer prove it issued no
 * device work (a phase-2 policy evaluation whose signatures
 * phase 1 already verified). Not in the reference: an observability hook. */
int bh_device_stats(uint64_t out[2]);

/* ---- Batched Hash -------------------------------------------------------------
 * CSP.Hash (bccsp/bccsp.go:109, bccsp/sw/impl.go:177-194) as a batch, and the
 * two SHA-256 checks of a pre-verified block's endorser transactions:
 *   - protoutil.CheckTxID (core/common/validation/msgvalidation.go:288-296):
 *     hex(SHA-256(nonce || creator)) == ChannelHeader.tx_id, as
 *     protoutil/proputils.go:351-370 computes it (BAD_PROPOSAL_TXID), and
 *   - the proposal hash (msgvalidation.go:228-241): SHA-256(channel_header ||
 *     action header || chaincode_proposal_payload) ==
 *     ProposalResponsePayload.proposal_hash, as protoutil/txutils.go:449-466
 *     (GetProposalHash2) computes it (INVALID_ENDORSER_TRANSACTION).
 * Record i is the nspan spans data[off[i*nspan + k], +len[i*nspan + k]), k <
 * nspan, hashed as one message in that order; a zero-length span contributes
 * nothing (its offset must still lie inside the buffer). alg is BH_HASH_SHA256
 * (Go crypto/sha256) or BH_HASH_SHA3_256 (x/crypto sha3.New256). SHA-384,
 * SHA-512 and SHA3-384 are not offered here: the wide SHA-2 digests exist on
 * the device only as the digest pass of the curve calls (BH_F_HASH_SHA384 /
 * BH_F_HASH_SHA512).
 * Outputs, either or both:
 *   digest[i]  32 bytes, the standard digest (hashlib's .digest())
 *   result[i]  the digest compared with the expected span data[want_off[i],
 *              +want_len[i]) under want_kind[i]:
 *                BH_HASH_WANT_RAW  equal iff want_len == 32 and the bytes match
 *                BH_HASH_WANT_HEX  equal iff want_len == 64 and the bytes are
 *                                  the lowercase hex of the digest (Go's
 *                                  hex.EncodeToString and a string compare:
 *                                  upper case does not match)
 *              any other kind is BH_HASH_MISMATCH.
 *   BH_HASH_RANGE (a span or the expected span ends beyond data_len): the
 *   record reads nothing and its digest is zeros.
 * bh_hash / bh_hash_submit take host memory. They check, before any device
 * work and with BH_E_INVALID and a bh_last_error text: alg; nspan in 1..3;
 * NULL b / data / off / len; digest and result both NULL; want_* partly NULL;
 * result without want_*; every span and expected span inside data_len (no sum
 * that can wrap), n <= 2^32 - 1. These checks need no device; BH_E_NOT_INIT
 * comes after them. n == 0 is BH_OK (a submit form still returns a job).
 * The batch runs on the first initialised device (no sharding), on a stream
 * of its own, not behind the compute lanes: a hash job submitted before a
 * verify call overlaps it. When `data` is the buffer the calling thread has
 * pre-staged (the block of bh_fabric_block_prevalidate), the records index
 * its device mirror and the data is not uploaded again; otherwise the call
 * uploads the bytes the records cover. bh_hash_submit's job is collected with
 * bh_verify_wait (exactly once, in any order among other jobs), which writes
 * digest / result; the caller's buffers stay valid and unchanged until then.
 * bh_device_stats counts a hash job as one batch and its n records.
 * bh_hash_dev: b is a host struct of DEVICE pointers on `device`, digest /
 * result device memory; stream NULL = the device's hash stream; sync != 0
 * waits. It cannot see the arrays, so the kernel's BH_HASH_RANGE is its guard
 * (data must lie in a device allocation: whole aligned dwords are loaded). */
#define BH_HASH_SHA256   1
#define BH_HASH_SHA3_256 2
#define BH_HASH_WANT_RAW 0
#define BH_HASH_WANT_HEX 1
#define BH_HASH_MATCH    0
#define BH_HASH_MISMATCH 1
#define BH_HASH_RANGE    2
typedef struct bh_hbatch {
  const uint8_t  *data;  size_t data_len;     /* every span indexes this buffer */
  const uint64_t *off;   const uint32_t *len; /* n * nspan, record-major */
  uint32_t nspan;                             /* 1..3 */
  const uint64_t *want_off; const uint32_t *want_len; const uint8_t *want_kind; /* or all NULL */
} bh_hbatch;
int bh_hash(int alg, const bh_hbatch *b, size_t n, uint8_t *digest /* n*32 or NULL */,
            uint8_t *result /* n or NULL */);
int bh_hash_submit(int alg, const bh_hbatch *b, size_t n, uint8_t *digest, uint8_t *result,
                   bh_job **job);             /* collected with bh_verify_wait */
int bh_hash_dev(int device, int alg, const bh_hbatch *b /* device pointers */, size_t n,
                uint8_t *digest, uint8_t *result, void *stream, int sync);

/* Host-side Go-exact DER unmarshal (bccsp/utils/ecdsa.go:41-65). Returns the
 * reason (BH_R_OK, BH_R_DER, BH_R_R_NONPOS, BH_R_S_NONPOS); on BH_R_OK fills
 * r, s (32-byte big-endian) or sets *r_big / *s_big when a value exceeds 256
 * bits. Pure host code, no device needed. */
int bh_parse_der_sig(const uint8_t *der, size_t len, uint8_t r[32], uint8_t s[32], int *r_big,
                     int *s_big);

/* ---- BDLS consensus messages -------------------------------------------
 * One record = one vendor/github.com/BDLS-bft/bdls/message.go SignedProto.
 * Verification restates SignedProto.Verify (message.go:170-184): hash =
 * SignedProto.Hash() (BLAKE2b-256 over "BDLS_CONSENSUS_SIGNATURE" || Version
 * u32-LE || X || Y || len(Message) u32-LE || Message, message.go:97-138), then
 * Go crypto/ecdsa.Verify with R, S = big.Int.SetBytes(R), SetBytes(S).
 * curve BH_CURVE_SECP256K1: as wired in orderer/consensus/bdls/chain.go:60-61
 * (Go verifyLegacy); BH_CURVE_P256: the curve-generic BDLS library with P-256
 * keys (verifyNISTEC). No low-S rule. Result reasons: BH_R_OK or a reject
 * code (every reject is Verify() == false). Off-curve / out-of-range keys are
 * rejected on both curves: BH_R_BAD_KEY on P-256 (pointFromAffine, before the
 * r, s ranges); on secp256k1, where verifyLegacy has no key check and rejects
 * such a record in the group equation, BH_R_MATH after the r, s ranges (BDLS
 * only admits registered participants' keys, consensus.go:456-466). */
typedef struct bh_bdls_batch {
  const uint8_t *xy;       /* n * 64: SignedProto.X || SignedProto.Y (32 B each)    */
  const uint8_t *r;        /* concatenated SignedProto.R (big-endian, any length)   */
  const uint64_t *r_off;
  const uint32_t *r_len;
  const uint8_t *s;        /* concatenated SignedProto.S                            */
  const uint64_t *s_off;
  const uint32_t *s_len;
  const uint32_t *version; /* SignedProto.Version                                   */
  const uint8_t *msg;      /* concatenated SignedProto.Message                      */
  const uint64_t *msg_off;
  const uint32_t *msg_len;
} bh_bdls_batch;

/* Host buffers, first initialised device (BDLS rounds are hundreds of records). */
int bh_verify_bdls(int curve, const bh_bdls_batch *b, size_t n, uint8_t *bitmap,
                   uint8_t *reason);
/* Device-resident; semantics of bh_verify_dev. */
int bh_verify_bdls_dev(int device, int curve, const bh_bdls_batch *b, size_t n,
                       uint64_t *bitmap_words, uint8_t *reason, void *stream, int sync,
                       bh_timing *timing);
/* As bh_verify_bdls_dev for callers that already hold SignedProto.Hash()
 * (consensus code that caches message hashes): msg[msg_off[i], +msg_len[i]) is
 * the hash itself and is not hashed again. e is Go's hashToInt / hashToNat of
 * those bytes for a 256-bit order: the left-most min(len, 32) bytes as a
 * big-endian integer, minus n once if >= n; length 0 gives e = 0. version is
 * not read (it may be NULL). Everything after the digest -- checks, reasons,
 * kernels, streams, timing -- is bh_verify_bdls_dev's. */
int bh_verify_bdls_prehashed_dev(int device, int curve, const bh_bdls_batch *b, size_t n,
                                 uint64_t *bitmap_words, uint8_t *reason, void *stream, int sync,
                                 bh_timing *timing);

/* ---- BDLS drained-batch pre-verification ------------------------------------
 * Replaces the per-message signature work of agent-tcp/tcp_peer.go:176-192
 * (inputConsensusMessage drains the queued raw messages and calls
 * Consensus.ReceiveMessage one by one) with ONE device batch: every
 * SignedProto reachable from the drained messages -- the outer one, each
 * Message.Proof of a <lock>/<select>/<decide>, Message.LockRelease and the
 * proofs of the <lock> it embeds, and (recursively, depth <= 8) the proofs a
 * <resync> pushes to the loopback -- is decoded (gogo/protobuf wire format,
 * message.pb.go Unmarshal semantics), gated on the participant set
 * (consensus.go:449-470) and verified with SignedProto.Verify semantics.
 *
 * results[i].status is the first failure among the checks that depend only on
 * the message bytes and the participant list, in the order Go runs them
 * (receiveMessage :1209-1226, verifyMessage :449-493, verifyLockMessage
 * :520-600, verifySelectMessage :628-728, verifyDecideMessage :829-902,
 * verifyLockReleaseMessage :604-623). Checks that need consensus state or
 * callbacks (height/round against the current round, StateValidate,
 * StateCompare, MessageValidator, the lock-release stage) are left to the
 * caller: status != BH_BDLS_OK means Go rejects the message for certain;
 * BH_BDLS_OK means the signature layer and proof structure pass. The quorum
 * checks (2t+1 proofs to the proposed state, <select> proposal counts) use
 * the default Config.StateHash (BLAKE2b-256 of the state, consensus.go:41);
 * pass BH_BDLS_F_NO_QUORUM with a custom StateHash.
 *
 * sp_reason (optional unless BH_BDLS_F_GIVEN_REASONS): one byte per decoded
 * SignedProto, message by message in the order [outer, proofs..., LockRelease,
 * its proofs..., resync sub-messages...] (results[i].sp_first / sp_count):
 * BH_R_OK, a BH_R_* reject, or BH_SP_NOT_VERIFIED (signer not a participant,
 * or the outer version is wrong). These feed a verified-signature cache that
 * the unchanged ReceiveMessage then consults.
 * *sp_total (required) receives the number of decoded SignedProtos; with
 * sp_reason != NULL and sp_cap < *sp_total the call fails with BH_E_INVALID
 * before any device work (call again with a larger buffer). */
#define BH_BDLS_F_GIVEN_REASONS 1u /* sp_reason is INPUT (e.g. cache hits): no device work */
#define BH_BDLS_F_NO_QUORUM 2u     /* skip the StateHash-based quorum checks */
#define BH_SP_NOT_VERIFIED 255

#define BH_BDLS_OK 0
#define BH_BDLS_DECODE 1                    /* proto.Unmarshal(SignedProto) failed, :1212 */
#define BH_BDLS_VERSION 2                   /* ErrMessageVersion, :1218 */
#define BH_BDLS_UNKNOWN_PARTICIPANT 3       /* ErrMessageUnknownParticipant, :469 */
#define BH_BDLS_BAD_SIGNATURE 4             /* ErrMessageSignature, :486 */
#define BH_BDLS_MSG_DECODE 5                /* proto.Unmarshal(Message) failed, :490 */
#define BH_BDLS_UNKNOWN_TYPE 6              /* ErrMessageUnknownMessageType */
#define BH_BDLS_EMPTY_STATE 7               /* Err{Lock,Decide}EmptyState */
#define BH_BDLS_NOT_LEADER 8                /* Err{Lock,Select,Decide}NotSignedByLeader */
#define BH_BDLS_PROOF_UNKNOWN_PARTICIPANT 9 /* Err*ProofUnknownParticipant */
#define BH_BDLS_PROOF_BAD_SIGNATURE 10      /* ErrMessageSignature from a proof */
#define BH_BDLS_PROOF_DECODE 11             /* a proof's Message does not decode */
#define BH_BDLS_PROOF_TYPE_MISMATCH 12      /* Err*ProofTypeMismatch */
#define BH_BDLS_PROOF_HEIGHT_MISMATCH 13    /* Err*ProofHeightMismatch */
#define BH_BDLS_PROOF_ROUND_MISMATCH 14     /* Err*ProofRoundMismatch */
#define BH_BDLS_PROOF_INSUFFICIENT 15       /* Err{Lock,Select,Decide}ProofInsufficient */
#define BH_BDLS_SELECT_STATE_MISMATCH 16    /* ErrSelectStateMismatch */
#define BH_BDLS_SELECT_PROOF_EXCEEDED 17    /* ErrSelectProofExceeded */
#define BH_BDLS_LOCKRELEASE_EMPTY 18        /* ErrMessageIsEmpty (nil LockRelease) */

typedef struct bh_bdls_msg_result {
  int32_t status;            /* BH_BDLS_* */
  int32_t bad_sp;            /* SignedProto (relative to sp_first) that failed, or -1 */
  uint32_t type;             /* Message.Type (valid from status >= BH_BDLS_UNKNOWN_TYPE or OK) */
  uint32_t distinct_signers; /* distinct participants among the checked proofs */
  uint64_t height;           /* Message.Height */
  uint64_t round;            /* Message.Round */
  uint32_t sp_first;         /* first SignedProto of this message in sp_reason */
  uint32_t sp_count;
} bh_bdls_msg_result;

/* msgs/msg_off/msg_len: n raw SignedProto encodings (host). participants:
 * n_participants * 64 bytes, Identity = X || Y (Config.Participants order,
 * which defines roundLeader). curve: BH_CURVE_SECP256K1 or BH_CURVE_P256. */
int bh_bdls_preverify(int curve, const uint8_t *msgs, const uint64_t *msg_off,
                      const uint32_t *msg_len, size_t n, const uint8_t *participants,
                      size_t n_participants, uint32_t flags, bh_bdls_msg_result *results,
                      uint8_t *sp_reason, size_t sp_cap, size_t *sp_total);

/* ---- Fabric block pre-verification ------------------------------------------
 * Replaces the per-signature bccsp Verify calls of one block's validation
 * (core/committer/txvalidator/v20/validator.go:180-265, validateTx :297-453)
 * with ONE device batch: the serialized common.Block is decoded (protobuf-go
 * wire rules), and for every transaction
 *   - the creator signature over Envelope.payload by SignatureHeader.creator
 *     (core/common/validation/msgvalidation.go:26-64, checked at :274), and
 *   - for ENDORSER_TRANSACTIONs each endorsement over
 *     proposal_response_payload || endorser by the endorser
 *     (core/common/validation/statebased/validator_keylevel.go:246-260),
 *     de-duplicated per identity exactly as common/policies/policy.go:363-395
 *     SignatureSetToValidIdentities does (a later signature of an identity
 *     is checked only while no earlier one of it verified)
 * are verified with identity.Verify semantics (msp/identities.go:170-199:
 * SHA-256, or SHA3-256 with BH_FAB_F_SHA3; Fabric's low-S rule). Identities
 * (msp.SerializedIdentity: PEM X.509) resolve to P-256 or P-384 keys
 * (id-ecPublicKey with prime256v1 or secp384r1) through a long-lived cache;
 * one this library cannot resolve (any other key) is reported, never guessed.
 * A P-384 identity's signatures are hashed with the same 256-bit family and
 * verified under its curve: a call that meets one sends its batch through
 * bh_verify_mixed, and one that meets none makes the P-256 call it always
 * made. The same holds for the signature-set, envelope and block-signature
 * entry points below. Checks that do not decide which signatures are verified
 * (CheckTxID, the proposal hash, channel / ledger state, policies) stay with
 * the unchanged validator, which consults the per-signature results
 * (bh_fabric_block_prevalidate below adds CheckTxID and the proposal hash).
 *
 * txs[i] (tx_cap >= number of transactions) and endorse[] (one byte per
 * endorsement, tx i's at [endorse_first, +endorse_count)); *n_tx and
 * *n_endorse are always set, and with too small buffers the call fails with
 * BH_E_INVALID before any device work. endorse[j]: BH_R_* when verified,
 * BH_FAB_E_DUPLICATE (skipped by the de-duplication), BH_FAB_E_BAD_IDENTITY,
 * or BH_SP_NOT_VERIFIED. */
#define BH_FAB_F_SHA3 1u      /* the MSPs' SignatureHashFamily is SHA3 */
#define BH_FAB_F_KEEP_KEYS 2u /* keys used >= 2 times get kept tables (BH_F_KEEP_KEYS); a
                                 resolved P-384 key is offered to the bh_keys384_* registry
                                 of every device at its second sighting, once (a full
                                 registry leaves it on the ladder; results never differ) */
#define BH_FAB_F_DECODE_ONLY 4u /* decode, resolve and plan only: no device work, every
                                   signature BH_SP_NOT_VERIFIED (host-side structure checks) */

#define BH_FAB_OK 0                 /* every check below passed */
#define BH_FAB_ENVELOPE 1           /* Envelope does not unmarshal: INVALID_OTHER_REASON (validator.go:310) */
#define BH_FAB_PAYLOAD 2            /* Payload does not unmarshal: BAD_PAYLOAD (msgvalidation.go:257-261) */
#define BH_FAB_HEADER 3             /* validateCommonHeader failed: BAD_COMMON_HEADER (:264-269) */
#define BH_FAB_CREATOR_IDENTITY 4   /* creator not resolvable here (Go's DeserializeIdentity decides) */
#define BH_FAB_CREATOR_SIGNATURE 5  /* creator.Verify failed (or nil signature): BAD_CREATOR_SIGNATURE */
#define BH_FAB_TX 6                 /* endorser-transaction structure: INVALID_ENDORSER_TRANSACTION */
#define BH_FAB_UNSUPPORTED 7        /* CONFIG_UPDATE envelope: UNSUPPORTED_TX_PAYLOAD */
#define BH_FAB_E_DUPLICATE 253
#define BH_FAB_E_BAD_IDENTITY 254

typedef struct bh_fab_tx {
  int32_t status;           /* BH_FAB_*: the first failing check in the validator's order */
  int32_t type;             /* ChannelHeader.type (0 if the header did not decode) */
  uint32_t creator;         /* BH_R_* of the creator signature, or BH_SP_NOT_VERIFIED */
  uint32_t endorse_first;   /* this transaction's endorsements in endorse[] */
  uint32_t endorse_count;
  uint32_t valid_endorsers; /* |SignatureSetToValidIdentities(endorsement set)| */
} bh_fab_tx;

int bh_fabric_block_preverify(const uint8_t *block, size_t len, uint32_t flags, bh_fab_tx *txs,
                              size_t tx_cap, size_t *n_tx, uint8_t *endorse, size_t endorse_cap,
                              size_t *n_endorse);

/* bh_fabric_block_preverify plus, per signature, where its inputs lie in the
 * block: the keys of the caller's verified-signature cache (INTEGRATION.md
 * sections 4-5), consulted by the unchanged checkSignatureFromCreator
 * (msgvalidation.go:26-64) and SignatureSetToValidIdentities (policy.go:
 * 363-395) with exactly (identity, signed bytes, signature). refs[i] (i <
 * *n_tx) is transaction i's creator signature (identity = SignatureHeader.
 * creator, signed bytes = Envelope.payload, signature = Envelope.signature;
 * ident_len 0 when the transaction has no creator to check); refs[*n_tx + j]
 * is endorsement j (identity = endorser, signed bytes = proposal_response_
 * payload || endorser, the SignedData of validator_keylevel.go:246-260).
 * Offsets are byte offsets into `block`; reason repeats txs[i].creator /
 * endorse[j]. *n_ref = *n_tx + *n_endorse; ref_cap must cover it. */
typedef struct bh_fab_sigref {
  uint64_t ident_off, sig_off, msg_off, msg2_off;
  uint32_t ident_len, sig_len, msg_len, msg2_len; /* signed bytes: msg || msg2 */
  uint32_t reason;                                /* BH_R_*, BH_FAB_E_*, BH_SP_NOT_VERIFIED */
  uint32_t reserved;
} bh_fab_sigref;
int bh_fabric_block_preverify_refs(const uint8_t *block, size_t len, uint32_t flags,
                                   bh_fab_tx *txs, size_t tx_cap, size_t *n_tx, uint8_t *endorse,
                                   size_t endorse_cap, size_t *n_endorse, bh_fab_sigref *refs,
                                   size_t ref_cap, size_t *n_ref);

/* bh_fabric_block_preverify_refs plus the two SHA-256 checks that
 * ValidateTransaction makes of an endorser transaction once its creator
 * signature verified, on the device (one bh_hash job over the block buffer,
 * submitted ahead of the signature batch on its own stream and collected
 * after it):
 *   - protoutil.CheckTxID (core/common/validation/msgvalidation.go:288-296):
 *     hex(SHA-256(nonce || creator)) == ChannelHeader.tx_id
 *     (protoutil/proputils.go:351-370), else BAD_PROPOSAL_TXID;
 *   - the proposal hash (msgvalidation.go:228-241): SHA-256(channel_header ||
 *     actions[0].header || chaincode_proposal_payload) ==
 *     ProposalResponsePayload.proposal_hash (GetProposalHash2,
 *     protoutil/txutils.go:449-466), else INVALID_ENDORSER_TRANSACTION.
 * Both are SHA-256 whatever the flags: ComputeTxID and GetProposalHash2 are
 * hard-wired to crypto/sha256, and BH_FAB_F_SHA3 changes only the signatures'
 * family. With them no host cryptography is left in ValidateTransaction for a
 * pre-validated block.
 * hashes[i] (tx_cap entries): txid is checked for every ENDORSER_TRANSACTION
 * whose common header validated; proposal_hash for those whose endorser-
 * transaction structure decoded, except that a chaincode_proposal_payload that
 * is absent or present with length 0 is nil in Go (protobuf-go's proto3 bytes
 * decoder stores append([]byte(nil), v...)): GetProposalHash2 answers "nil
 * arguments", so that transaction is BH_FAB_TX with proposal_hash =
 * BH_FAB_H_NOT_CHECKED. CONFIG / CONFIG_UPDATE transactions and anything that
 * failed earlier in the decode get BH_FAB_H_NOT_CHECKED for both. The spans
 * nonce / creator / txid / chdr are filled once the common header validated
 * (any type), ashdr / ccpp / phash once the endorser-transaction structure
 * decoded; len 0 = the decode never reached it (or the field is empty).
 * txs[i].status is the first failing check in Go's order: ENVELOPE / PAYLOAD /
 * HEADER / CREATOR_IDENTITY / CREATOR_SIGNATURE / UNSUPPORTED as before, then
 * BH_FAB_TXID, BH_FAB_TX, BH_FAB_PROPOSAL_HASH. txs[i].type / creator /
 * endorse_* / valid_endorsers, endorse[] and refs[] are exactly what
 * bh_fabric_block_preverify_refs gives for the same block and flags. refs may
 * be NULL (*n_ref is still set when n_ref is given). With
 * BH_FAB_F_DECODE_ONLY the spans are filled, both checks are
 * BH_FAB_H_NOT_CHECKED and the statuses are the old call's. A consumer keys
 * hashes[i] like the signature cache and falls back to the Go checks on
 * BH_FAB_H_NOT_CHECKED. */
#define BH_FAB_TXID 8            /* CheckTxID failed: BAD_PROPOSAL_TXID (msgvalidation.go:288-296) */
#define BH_FAB_PROPOSAL_HASH 9   /* proposal hash differs: INVALID_ENDORSER_TRANSACTION (:228-241) */
#define BH_FAB_H_NOT_CHECKED 0xff
typedef struct bh_fab_txhash {
  uint8_t txid, proposal_hash;   /* BH_HASH_MATCH / BH_HASH_MISMATCH / BH_FAB_H_NOT_CHECKED */
  uint8_t reserved[6];
  /* where the inputs lie in `block` (len 0 = the decode never reached it) */
  uint64_t nonce_off, creator_off, txid_off, chdr_off, ashdr_off, ccpp_off, phash_off;
  uint32_t nonce_len, creator_len, txid_len, chdr_len, ashdr_len, ccpp_len, phash_len, pad;
} bh_fab_txhash;
int bh_fabric_block_prevalidate(const uint8_t *block, size_t len, uint32_t flags,
    bh_fab_tx *txs, size_t tx_cap, size_t *n_tx, uint8_t *endorse, size_t endorse_cap,
    size_t *n_endorse, bh_fab_sigref *refs, size_t ref_cap, size_t *n_ref, /* refs may be NULL */
    bh_fab_txhash *hashes /* tx_cap entries */);

/* ---- signature sets: SignatureSetToValidIdentities as a batch ------------------
 * common/policies/policy.go:363-395, the batch point of every policy
 * evaluation (cauthdsl, implicit-meta sub-policies, the endorsement policy,
 * SigFilter, block signatures): for each signature set, in order, an entry
 * whose identity does not deserialize is skipped, an entry of an identity
 * already validated earlier in the set is skipped (de-duplication by Mspid +
 * Id, Id over the sanitized certificate), every other entry is verified with
 * identity.Verify (hash of data, then Verify, low-S). Sets are [set_first[k],
 * set_first[k+1]) (the last ends at n). result[i]: BH_R_* when verified,
 * BH_FAB_E_DUPLICATE, BH_FAB_E_BAD_IDENTITY, or BH_SP_NOT_VERIFIED;
 * valid_identities[k] = the number of identities the set yields. Flags:
 * BH_FAB_F_SHA3 / BH_FAB_F_KEEP_KEYS / BH_FAB_F_DECODE_ONLY. */
typedef struct bh_sd_batch { /* protoutil.SignedData {Identity, Data, Signature}, SoA */
  const uint8_t *identity;   /* msp.SerializedIdentity bytes */
  const uint64_t *identity_off;
  const uint32_t *identity_len;
  const uint8_t *data;       /* the signed bytes */
  const uint64_t *data_off;
  const uint32_t *data_len;
  const uint8_t *sig;        /* DER signatures */
  const uint64_t *sig_off;
  const uint32_t *sig_len;
} bh_sd_batch;
int bh_signature_sets_verify(const bh_sd_batch *b, size_t n, const uint32_t *set_first,
                             size_t n_sets, uint32_t flags, uint8_t *result,
                             uint32_t *valid_identities);

/* Orderer broadcast SigFilter (orderer/common/msgprocessor/sigfilter.go:50-80)
 * for n serialized common.Envelopes: EnvelopeAsSignedData
 * (protoutil/signeddata.go:60-86) then the one-signature set of the policy.
 * status[i]: BH_FAB_OK, BH_FAB_ENVELOPE, BH_FAB_PAYLOAD, BH_FAB_HEADER
 * ("Missing Header" / signature header), BH_FAB_CREATOR_IDENTITY,
 * BH_FAB_CREATOR_SIGNATURE; reason[i]: BH_R_* or BH_SP_NOT_VERIFIED. */
int bh_envelopes_preverify(const uint8_t *envs, const uint64_t *env_off, const uint32_t *env_len,
                           size_t n, uint32_t flags, int32_t *status, uint8_t *reason);

/* Block signatures (protoutil/blockutils.go:245-300 BlockSignatureVerifier,
 * non-BFT form, as orderer/common/cluster/util.go:300 VerifyBlockSignature and
 * the peer's gossip MCS run it) for n serialized blocks: per block the
 * SIGNATURES metadata's signature set, signed data = Metadata.value ||
 * signature_header || BlockHeaderBytes(header) (ASN.1 DER of number,
 * previous_hash, data_hash), de-duplicated as above. sig_reason[]:
 * one byte per MetadataSignature, block i's at [sig_first, +sig_count). */
#define BH_BLK_OK 0
#define BH_BLK_DECODE 1            /* block does not unmarshal or has no header */
#define BH_BLK_NO_SIGNATURES 2     /* "no signatures in block metadata" */
#define BH_BLK_METADATA 3          /* Metadata does not unmarshal */
#define BH_BLK_SIGNATURE_HEADER 4  /* a signature header does not unmarshal */
#define BH_BLK_IDENTIFIER_HEADER 5 /* BFT: an IdentifierHeader does not unmarshal */
#define BH_FAB_E_NOT_CONSENTER 252 /* BFT: identifier outside the consenter set (not in the set) */
typedef struct bh_blocksig_result {
  int32_t status;            /* BH_BLK_* */
  uint32_t sig_first;
  uint32_t sig_count;
  uint32_t valid_identities; /* identities the policy evaluation receives */
} bh_blocksig_result;
int bh_block_signatures_preverify(const uint8_t *blocks, const uint64_t *block_off,
                                  const uint32_t *block_len, size_t n, uint32_t flags,
                                  bh_blocksig_result *res, uint8_t *sig_reason, size_t sig_cap,
                                  size_t *sig_total);

/* BFT form (protoutil/blockutils.go:245-308 with bftEnabled, the V3_0 channel
 * capability, common/capabilities/channel.go:111; this fork registers BDLS as
 * consensus type "BFT", orderer/common/server/main.go:628). With
 * BH_BLK_F_BFT, a MetadataSignature whose signature_header is empty and whose
 * identifier_header is not is signed by the consenter with that identifier
 * (the FIRST cb.Consenter with Id == IdentifierHeader.identifier; identity =
 * marshalled msp.SerializedIdentity{MspId, Identity}) over Metadata.value ||
 * identifier_header || BlockHeaderBytes; an identifier outside the set is
 * skipped by Go (reported BH_FAB_E_NOT_CONSENTER, not part of the set's
 * de-duplication), and an IdentifierHeader that does not unmarshal fails the
 * block (BH_BLK_IDENTIFIER_HEADER). Without the flag (or with the signature
 * header present) this is bh_block_signatures_preverify. consenters may be
 * NULL (an empty set). */
#define BH_BLK_F_BFT 8u
typedef struct bh_consenter_set { /* cb.Consenter{Id, MspId, Identity}, SoA */
  const uint32_t *id;
  const uint8_t *msp_id;     /* MspId strings (not NUL-terminated) */
  const uint64_t *msp_id_off;
  const uint32_t *msp_id_len;
  const uint8_t *identity;   /* Identity bytes (PEM certificate) */
  const uint64_t *identity_off;
  const uint32_t *identity_len;
  size_t n;
} bh_consenter_set;
int bh_block_signatures_preverify_bft(const uint8_t *blocks, const uint64_t *block_off,
                                      const uint32_t *block_len, size_t n, uint32_t flags,
                                      const bh_consenter_set *consenters, bh_blocksig_result *res,
                                      uint8_t *sig_reason, size_t sig_cap, size_t *sig_total);

/* ---- X.509 certificate signatures ---------------------------------------------
 * Certificate i's signature against issuer key i (X || Y): Go crypto/x509
 * Certificate.CheckSignatureFrom for an ECDSA issuer (checkSignature: SHA-256
 * of the raw TBSCertificate, then ecdsa.VerifyASN1 -- cryptobyte-strict DER,
 * r, s in [1, n-1], NO low-S rule), the per-link check of the MSP's chain
 * validation (msp/mspimpl.go:717-722 cert.Verify, msp/cert.go:76-116). The
 * TBS bytes are hashed on the device straight out of the caller's buffer.
 * reason: BH_R_OK, BH_R_DER (signature not strict DER), BH_R_R_NONPOS /
 * BH_R_S_NONPOS (zero), BH_R_BAD_KEY, BH_R_R_RANGE / BH_R_S_RANGE, BH_R_MATH,
 * or BH_R_UNSUPPORTED (not ecdsa-with-SHA256, inner/outer algorithm mismatch,
 * or not a certificate this parser walks). */
int bh_verify_x509(const uint8_t *certs, const uint64_t *cert_off, const uint32_t *cert_len,
                   const uint8_t *issuer_pub, size_t n, uint8_t *bitmap, uint8_t *reason);

/* bh_verify_x509 for issuers on either NIST curve of the sw provider and the
 * three SHA-2 algorithms crypto/x509 signs ECDSA certificates with (a P-384 CA
 * key makes x509.CreateCertificate, and fabric-ca with it, choose
 * ecdsa-with-SHA384). Record i's issuer key is bh_curve_key_bytes(
 * issuer_curve[i]) bytes at issuer_pub + issuer_pub_off[i]; issuer_curve[i] is
 * BH_CURVE_P256 or BH_CURVE_P384, anything else BH_E_INVALID for the call.
 * Accepted, with inner and outer OID equal: ecdsa-with-SHA256
 * (1.2.840.10045.4.3.2), -SHA384 (4.3.3), -SHA512 (4.3.4); the hash comes from
 * the algorithm and the curve from the key, independently (checkSignature), so
 * all six pairings verify: e is the leftmost 32 / 48 bytes of the digest.
 * Everything else is BH_R_UNSUPPORTED. After the algorithm check the semantics
 * and reason codes are those of bh_verify_x509, with r, s in [1, n-1] for the
 * issuer's n. Records are grouped by (curve, hash) and each group runs through
 * bh_verify with BH_F_NO_LOW_S and the group's BH_F_HASH_* flag. */
int bh_verify_x509_ex(const uint8_t *certs, const uint64_t *cert_off, const uint32_t *cert_len,
                      const uint8_t *issuer_pub, const uint64_t *issuer_pub_off,
                      const uint8_t *issuer_curve, size_t n, uint8_t *bitmap, uint8_t *reason);

/* ---- device buffers on an initialised device (callers that keep batches
 * resident in HBM, e.g. bench.py; the library owns the HIP runtime so callers
 * never mix runtimes). Copies are synchronous on the device's stream. ---- */
int bh_dev_alloc(int device, size_t bytes, void **ptr);
int bh_dev_free(int device, void *ptr);
int bh_memcpy_h2d(int device, void *dst, const void *src, size_t bytes);
int bh_memcpy_d2h(int device, void *dst, const void *src, size_t bytes);
int bh_sync(int device); /* wait for all work queued on the device's library stream */

/* Deferred stage timing for pipelined callers: after bh_timing_begin, every
 * pass on `device` that is given no bh_timing records HIP events around its
 * stages on its launch stream WITHOUT synchronising; bh_timing_end waits for
 * those events and returns the stage times summed over the passes since
 * begin (routing counts and lanes of the last pass). */
int bh_timing_begin(int device);
int bh_timing_end(int device, bh_timing *timing);

/* ---- key registry ---------------------------------------------------------
 * Per device and curve, a persistent store of per-key fixed-base tables
 * (65 x 8 multiples of Q, 56 KiB per key in HBM). A record whose public key
 * is registered skips every doubling: u2 Q is 65 table additions. This is the
 * device-side counterpart of the reference's long-lived identities -- the
 * MSP identity cache (msp/cache/cache.go) for Fabric, the fixed participant
 * set (consensus.go:456-466, Config.Participants) for BDLS. Verification
 * results never depend on the registry (same bitmap and reasons with or
 * without it); only the route and the time do.
 * capacity: tables per (device, curve); bh_keys_register / BH_F_KEEP_KEYS
 * reserve 65536 on first use when not reserved before. Entries persist until
 * bh_keys_clear; once full, new keys take the per-batch path. */
int bh_keys_reserve(int device, int curve, size_t capacity);
/* Import and register n keys (host pointer, n * 64 bytes X || Y). status
 * (optional, n bytes): 0 registered (or already present), BH_R_BAD_KEY not a
 * valid curve point, 255 registry full. Synchronous. */
int bh_keys_register(int device, int curve, const uint8_t *pub, size_t n, uint8_t *status);
int bh_keys_clear(int device, int curve);
int bh_keys_count(int device, int curve, size_t *count);

/* ---- key registry, BH_CURVE_P384 ---------------------------------------------
 * The P-384 counterpart of the registry above, with entry points of its own:
 * 96-byte keys, and per key a fixed-base table of 96 windows x 15 multiples of
 * Q (161,280 bytes in HBM, plus the 96 key bytes). A P-384 record whose key is
 * registered skips the ladder: u2 Q and u1 G are table additions, about 2,000
 * field products against the ladder's 5,600. As above this mirrors the
 * reference's long-lived identities -- the MSP identity cache
 * (msp/cache/cache.go) for Fabric, the fixed participant set
 * (consensus.go:456-466, Config.Participants) for BDLS -- and results never
 * depend on it: same bitmap and reasons with or without, in bh_verify and
 * bh_verify_dev, with any BH_F_HASH_* flag. BH_F_KEEP_KEYS stays ignored for
 * P-384: kept tables are built by bh_keys384_register alone, never by a pass
 * (without BH_F_BATCH_KEYS bh_timing.n_keytables stays 0; n_keycomb counts the records that took the
 * table route, plan_ms the lookup, keycomb_ms the table route, build_ladder_ms
 * the ladder; the two routes run side by side after the lookup, so these two
 * times overlap). bh_keys_* above keep refusing BH_CURVE_P384.
 * device: -1 means every initialised device. A null pub with n > 0 or a null
 * count is BH_E_INVALID; otherwise, before bh_init, BH_E_NOT_INIT.
 * capacity: keys per device, 1 .. 65536; reserving replaces (and empties) the
 * registry. bh_keys384_register reserves 256 (39.4 MiB) when nothing was
 * reserved before. Entries persist until bh_keys384_clear or bh_shutdown; once
 * full, new keys stay on the ladder. */
int bh_keys384_reserve(int device, size_t capacity);
/* Import and register n keys (host pointer, n * 96 bytes X || Y). status
 * (optional, n bytes): 0 registered (or already present), BH_R_BAD_KEY not a
 * point of P-384 (X or Y >= p, or off the curve: the checks a pass makes),
 * 255 registry full. Synchronous: under the device lock, behind every lane's
 * work and every P-384 pass; the tables are complete when it returns. */
int bh_keys384_register(int device, const uint8_t *pub, size_t n, uint8_t *status);
int bh_keys384_clear(int device);
/* Keys registered; with device -1 the minimum over the devices. */
int bh_keys384_count(int device, size_t *count);

#ifdef __cplusplus
}
#endif
#endif /* BDLS_HIP_H */
