/* ldgpu.h -- C ABI of libldgpu.so, the MI355X (gfx950) hot path of
 * spark-languagedetector: FIT byte n-gram counting into per-language gram
 * probability tables, and SCORE (window scan, gram->row lookup, fp64
 * accumulation, argmax).
 *
 * Plain C, POD arguments only.  Every entry point returns an int status
 * (LDGPU_OK = 0) and leaves a thread-local message for ldgpu_last_error().
 * All entry points are thread-safe; calls on one ldgpu_ctx are serialised on
 * that context's HIP stream.
 *
 * Reference interfaces replaced (Scala, /root/reference/src/main/scala/org/
 * apache/spark/ml/feature/languagedetection/):
 *   ldgpu_model_create  -- new LanguageDetectorModel(gramProbabilities,
 *                          gramLengths, languages)  LanguageDetectorModel.scala:178-198
 *                          + the table broadcast of transform  :222
 *   ldgpu_score[_device]-- LanguageDetectorModel.detect(Array[Byte], map, langs,
 *                          grams) :131-156, batched over documents (the per-row
 *                          map of transform :225-238)
 *   ldgpu_count[_device]-- LanguageDetector computeGrams + reduceGrams
 *                          LanguageDetector.scala:25-66
 *   ldgpu_fit_table_*   -- computeProbabilities + filterTopGrams + collect.toMap
 *                          LanguageDetector.scala:75-132, :252-254
 *
 * Encodings are the caller's job (as in the reference): FIT documents are
 * UTF-8 bytes (String.getBytes(UTF-8), LanguageDetector.scala:37); SCORE
 * documents are the low byte of every UTF-16 code unit
 * (text.toCharArray.map(_.toByte), LanguageDetectorModel.scala:161).
 *
 * Documents are packed: bytes[offsets[d] .. offsets[d+1]) is document d;
 * offsets has n_docs + 1 non-decreasing entries.
 */
#ifndef LDGPU_H
#define LDGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum ldgpu_status {
    LDGPU_OK = 0,
    LDGPU_EINVAL = 1,        /* bad argument: gram length <= 0, bad offsets, null pointer, L < 1 */
    LDGPU_EROWLEN = 2,       /* a scored window hit a row whose length != #languages
                                (BLAS.axpy require, LanguageDetectorModel.scala:149) */
    LDGPU_ENOMEM = 3,        /* device or host allocation failed / count table full */
    LDGPU_EDEVICE = 4,       /* HIP runtime error */
    LDGPU_EUNSUPPORTED = 5,  /* outside the device path's limits (see below) */
    LDGPU_ENODEV = 6         /* no HIP device */
};

/* Device-path limits.  Gram lengths 1..LDGPU_MAX_GRAM for SCORE tables and
 * LDGPU_MAX_FIT_GRAM for FIT counting: keys of up to 7 bytes pack into one
 * u64 (7 payload bytes + a length byte); keys of 8..15 bytes take two words,
 * in a table of their own (SCORE and FIT alike); a SCORE table with a gram
 * length beyond 15 keeps every key in a general table (hash + key bytes
 * compared on the device: any length, as the reference), and FIT counts grams
 * of more than 15 bytes in a table of such keys (up to 2^24 - 1 bytes).  1..LDGPU_MAX_LANGS
 * languages (SCORE scores more than 256 in blocks of 256 languages). */
#define LDGPU_MAX_GRAM 2147483647  /* SCORE tables: any gram length */
#define LDGPU_MAX_FIT_GRAM 16777215  /* FIT counting: lengths beyond 15 in a general-key table */
#define LDGPU_MAX_LANGS 4096
#define LDGPU_MAX_GRAM_LENGTHS 32

const char* ldgpu_version(void);
/* build provenance: sha256 (first 16 hex digits) of the sources this library
 * was compiled from (spark-languagedetector_amd/Makefile, PROV) */
const char* ldgpu_build_id(void);
const char* ldgpu_last_error(void);          /* thread-local, never NULL */
int ldgpu_device_count(int32_t* out_count);

/* ---------------------------------------------------------------- context */
typedef struct ldgpu_ctx ldgpu_ctx;
int ldgpu_ctx_create(int32_t device, ldgpu_ctx** out);
int ldgpu_ctx_destroy(ldgpu_ctx* ctx);
int ldgpu_ctx_synchronize(ldgpu_ctx* ctx);
void* ldgpu_ctx_stream(ldgpu_ctx* ctx);      /* the context's hipStream_t */

/* Page-locked host memory for the host-buffer APIs: documents packed straight
 * into it (a JNI shim wraps it in direct ByteBuffers) are copied to the device
 * without a staging copy; labels written into it skip one too.  Replaces the
 * JVM-owned row buffers of transform (LanguageDetectorModel.scala:225-238). */
int ldgpu_host_alloc(ldgpu_ctx* ctx, int64_t n_bytes, void** out);
int ldgpu_host_free(ldgpu_ctx* ctx, void* p);

/* ------------------------------------------------------------------ SCORE */
typedef struct ldgpu_model ldgpu_model;

/* The gram -> probability-row map.  Key i is key_bytes[key_offsets[i] ..
 * key_offsets[i+1]); its row is rows[i*n_langs .. (i+1)*n_langs) in
 * supported-language order.  row_ok (nullable) marks rows whose length in the
 * caller's map differs from n_langs: scoring a document that hits such a row
 * fails with LDGPU_EROWLEN, as BLAS.axpy does in the reference.  A later
 * duplicate key replaces an earlier one (Scala toMap).  gram_lengths is kept
 * in order, duplicates included (each repeat scans the document again). */
int ldgpu_model_create(ldgpu_ctx* ctx, int64_t n_rows, const uint8_t* key_bytes,
                       const int64_t* key_offsets, const double* rows, const uint8_t* row_ok,
                       int32_t n_langs, const int32_t* gram_lengths, int32_t n_grams,
                       ldgpu_model** out);
/* Mask form of the same table (what a fit produces, and what a table too
 * large for dense rows is carried in): row i is vals[i] at the languages set
 * in masks[i*S .. (i+1)*S), S = ceil(n_langs / 64), 0.0 elsewhere. */
int ldgpu_model_create_masks(ldgpu_ctx* ctx, int64_t n_rows, const uint8_t* key_bytes,
                             const int64_t* key_offsets, const uint64_t* masks, const double* vals,
                             int32_t n_langs, const int32_t* gram_lengths, int32_t n_grams,
                             ldgpu_model** out);
int ldgpu_model_destroy(ldgpu_model* model);

/* mode: 0 = every row is one value times a language bitmask, 1 = dense fp64
 * rows, 2 = mask form where every row shares ONE finite value (fit-produced
 * tables whose grams all have the same presence class, e.g. all unique to one
 * language): scored from per-language hit counts.  n_keys: keys resident on
 * the device. */
int ldgpu_model_info(const ldgpu_model* model, int32_t* mode, int64_t* n_keys,
                     int64_t* table_slots, int64_t* filter_bits, int64_t* device_bytes);

/* The device layout the model's scoring kernel takes (bit set = in use), so a
 * caller (and the parity tests) can tell which product path scores it:
 * the window filter (LDS prefix Bloom, or a keyed bloom in L2 / Infinity Cache,
 * one word per key or one 64-B line per window position), the key table
 * (cuckoo slots, or 4-slot buckets for count-mode tables beyond 2^20 keys),
 * packs of short documents (labels-only count mode). */
#define LDGPU_LAYOUT_LDS_BLOOM          0x01
#define LDGPU_LAYOUT_KEYED_BLOOM        0x02
#define LDGPU_LAYOUT_KEYED_BLOOM_LINES  0x04
#define LDGPU_LAYOUT_BUCKETS            0x08
#define LDGPU_LAYOUT_WIDE_KEYS          0x10
#define LDGPU_LAYOUT_DIRECT             0x20
#define LDGPU_LAYOUT_PACKS              0x40
#define LDGPU_LAYOUT_LANG_BLOCKS        0x80
#define LDGPU_LAYOUT_GENERAL_KEYS       0x100  /* keys of any length (a gram length > 15) */
#define LDGPU_LAYOUT_KEYED_BLOOM_CHUNKS 0x200  /* count mode: one 16-B bloom chunk per window position */
#define LDGPU_LAYOUT_CLASSES            0x400  /* labels-only calls on a mask table of at most 4 distinct
                                                  finite values: per-(value, language) hit counts and a
                                                  rounding bound; documents the bound cannot separate
                                                  replayed in reference order */
#define LDGPU_LAYOUT_NARROW_SLOTS       0x800  /* order-free scoring (count / class mode, LDS Bloom): the keys
                                                  of 3 and 4 bytes verified from a second table of 8-byte
                                                  slots (no key of 5 bytes or more, one language per such
                                                  row) */
#define LDGPU_LAYOUT_TRIE               0x1000 /* count mode, labels-only calls on documents that are not
                                                  packed: every key (at most 4 bytes, one language each) in
                                                  an exact byte trie held in LDS; no filter, queue or verify */
#define LDGPU_LAYOUT_TRIE_SUM           0x2000 /* set beside LDGPU_LAYOUT_TRIE: the trie's path-sum form --
                                                  every root path names one language (at most 63 languages)
                                                  and counts at most 4, so a node says what its whole path
                                                  counts and a window position is counted once */
#define LDGPU_LAYOUT_TRIE_PAIR          0x4000 /* set beside LDGPU_LAYOUT_TRIE and _TRIE_SUM: the path-sum
                                                  form with one counter per (language, count W) pair, a
                                                  node holding its counter's offset (largest W times the
                                                  language count at most 63) */
int ldgpu_model_layout(const ldgpu_model* model, int32_t* flags);
/* The model's language count (a caller sizing score buffers, e.g. the JNI
 * shim, takes it from the model rather than trusting its own). */
int ldgpu_model_langs(const ldgpu_model* model, int32_t* n_langs);

/* Host buffers in, host buffers out; synchronous.  out_scores is nullable
 * ([n_docs][n_langs] fp64).  out_labels[d] is the index into the supported
 * languages of argmax(scores of d): first maximum, all-zero -> 0.  Chunks of
 * documents are pipelined over two streams (copy-in / score / copy-out of one
 * chunk overlap the host staging of the next); buffers from ldgpu_host_alloc
 * are copied from / to directly, pageable ones through pinned staging.  (A
 * class-mode table's replay of ambiguous documents is sized on the device, so
 * the pipeline never waits for the GPU between chunks.) */
int ldgpu_score(ldgpu_model* model, const uint8_t* bytes, const int64_t* offsets,
                int64_t n_docs, int32_t* out_labels, double* out_scores);

/* Device-resident variant, asynchronous on `stream` (a hipStream_t used as
 * given: NULL is HIP's null stream; ldgpu_ctx_stream() gives the context's).
 * d_bytes must be 4-byte aligned and n_bytes >= d_offsets[n_docs].
 * d_scores is nullable.  Offsets are trusted (validate with the host API);
 * documents must be shorter than 2^28 bytes (the host API checks this).
 * A labels-only call (d_scores NULL) on a model in class mode
 * (LDGPU_LAYOUT_CLASSES) replays the documents its rounding bound left
 * ambiguous on the same stream, sized on the device: it is asynchronous too. */
int ldgpu_score_device(ldgpu_model* model, const uint8_t* d_bytes, int64_t n_bytes,
                       const int64_t* d_offsets, int64_t n_docs, int32_t* d_labels,
                       double* d_scores, void* stream);

/* Top-k form of SCORE: per document the k best languages in order
 * (out_top_labels [n_docs][k]) and, out_top_scores given ([n_docs][k],
 * nullable), their fp64 scores bit for bit (a -0.0 stays -0.0, a NaN a NaN).
 * The selection runs on the device: only [n_docs][k] leaves it.
 * 1 <= k <= min(n_langs, LDGPU_MAX_TOPK), anything else is LDGPU_EINVAL.
 * Order of a document's scores s[0 .. n_langs): language i comes before j if
 * s[i] > s[j], or if they compare equal and i < j, where
 *   -0.0 equals +0.0;
 *   a NaN at index 0 comes first;
 *   a NaN at any other index comes after every non-NaN value (-inf included),
 *   NaNs among themselves by ascending index.
 * Entry 0 is therefore the label ldgpu_score gives (breeze's first maximum,
 * LanguageDetectorModel.scala:154); a document without a hit yields the labels
 * 0, 1, .., k-1 with scores 0.0.  The reference has no such output.
 * Argument checks, LDGPU_EROWLEN and the document-length limit, thread safety
 * and the pipeline over pinned / pageable buffers are those of ldgpu_score. */
#define LDGPU_MAX_TOPK 16
int ldgpu_score_topk(ldgpu_model* model, const uint8_t* bytes, const int64_t* offsets,
                     int64_t n_docs, int32_t k, int32_t* out_top_labels, double* out_top_scores);

/* Device-resident variant, asynchronous on `stream` under the rules of
 * ldgpu_score_device.  d_top_labels [n_docs][k], d_top_scores nullable
 * [n_docs][k].  The documents are scored in chunks into stream-ordered
 * scratch (at most 256 MiB of scores, chunk x n_langs doubles) and each chunk's
 * rows selected from there: the full score matrix never exists. */
int ldgpu_score_topk_device(ldgpu_model* model, const uint8_t* d_bytes, int64_t n_bytes,
                            const int64_t* d_offsets, int64_t n_docs, int32_t k,
                            int32_t* d_top_labels, double* d_top_scores, void* stream);

/* Span form of SCORE, for mixed-language documents: every document is cut on
 * the device into overlapping spans of `width` bytes every `stride` bytes, and
 * every span is scored as a document of its own.  The reference has no such
 * output.  width >= 1 and 1 <= stride <= width, anything else is LDGPU_EINVAL;
 * width >= 2^28 (the document limit of ldgpu_score) is LDGPU_EUNSUPPORTED.
 *   Spans of a document of len bytes: one if len <= width, otherwise
 *   1 + ceil((len - width) / stride).  Span j is bytes [j stride,
 *   min(j stride + width, len)) of the document: every span of a document
 *   longer than width holds at least one byte; an empty document has one
 *   empty span.
 *   The label and the score row of a span are exactly what ldgpu_score gives
 *   for a document holding that slice: partial windows of a slice shorter
 *   than a gram length, label 0 without a hit, the tie and NaN rules, scores
 *   bit for bit.
 *   Spans are numbered document by document: span_offsets[d] is the index of
 *   document d's first span, span_offsets[0] = 0 and span_offsets[n_docs] the
 *   number of spans (int64: at stride 1 of the order of the corpus bytes).
 * ldgpu_span_offsets is host arithmetic (no context, no GPU; the offsets are
 * checked as by ldgpu_score); ldgpu_span_offsets_device the same on device
 * arrays, asynchronous on `stream`, offsets trusted. */
int ldgpu_span_offsets(const int64_t* offsets, int64_t n_docs, int32_t width, int32_t stride,
                       int64_t* span_offsets /* [n_docs + 1] */);
int ldgpu_span_offsets_device(ldgpu_ctx* ctx, const int64_t* d_offsets, int64_t n_docs, int32_t width,
                              int32_t stride, int64_t* d_span_offsets, void* stream);

/* Host buffers in and out; synchronous and thread-safe as ldgpu_score.
 * out_labels [n_spans], out_scores nullable [n_spans][n_langs], n_spans =
 * span_offsets[n_docs] of ldgpu_span_offsets.  Argument checks, LDGPU_EROWLEN
 * (raised when a window inside some span hits a wrong-length row) and the
 * pipeline over pinned / pageable buffers are those of ldgpu_score -- except
 * the document-length limit: only spans are scored, so a document may have
 * 2^28 bytes and more.  Only the documents' bytes cross to the device, never
 * the width / stride expansion. */
int ldgpu_score_spans(ldgpu_model* model, const uint8_t* bytes, const int64_t* offsets, int64_t n_docs,
                      int32_t width, int32_t stride, int32_t* out_labels, double* out_scores);

/* Device-resident variant, asynchronous on `stream` under the rules of
 * ldgpu_score_device (d_bytes 4-byte aligned, n_bytes >= d_offsets[n_docs],
 * offsets trusted; documents of any length).  d_span_offsets [n_docs + 1] is
 * ldgpu_span_offsets_device's output for the same width and stride, n_spans
 * its last entry (which the caller knows, or bounds: a span index at or
 * beyond d_span_offsets[n_docs] is scored as an empty span, label 0).
 * d_labels [n_spans], d_scores nullable [n_spans][n_langs].  The spans are
 * gathered in chunks (at most 64 MiB of span bytes, 2^20 spans) into
 * stream-ordered scratch and scored from there; nothing is read back. */
int ldgpu_score_spans_device(ldgpu_model* model, const uint8_t* d_bytes, int64_t n_bytes,
                             const int64_t* d_offsets, int64_t n_docs, int32_t width, int32_t stride,
                             const int64_t* d_span_offsets, int64_t n_spans,
                             int32_t* d_labels, double* d_scores, void* stream);

/* Segment form of SCORE: the span labels of every document smoothed by a best
 * path over its spans with a cost per language change, computed on the device
 * (only the [n_spans] labels leave it; the score matrix never exists).  The
 * reference has no such output.  Spans, their numbering and their score rows
 * s_j[0 .. n_langs) are exactly those of ldgpu_score_spans; penalty is an
 * fp64 >= 0 (+inf allowed; negative or NaN is LDGPU_EINVAL) in score units --
 * a span's score is a sum of log(1 + 1/k) per hit window.  The rule, for a
 * document's spans 0 .. n-1 (L = n_langs):
 *   first_max(v):  m = v[0], a = 0;
 *                  for l = 1 .. L-1: if (v[l] > m) { m = v[l]; a = l; }  -> (m, a)
 *   dp_0[l]    = s_0[l]
 *   (m_j, a_j) = first_max(dp_j)
 *   for j >= 1, with t = m_{j-1} - penalty (one fp64 subtraction):
 *     switch_j[l] = (t > dp_{j-1}[l])      (a tie stays; any comparison with a NaN stays)
 *     dp_j[l]     = s_j[l] + (switch_j[l] ? t : dp_{j-1}[l])      (one fp64 addition)
 *   y_{n-1} = a_{n-1};   y_{j-1} = switch_j[y_j] ? a_{j-1} : y_j   for j = n-1 .. 1
 * y_j is span j's label.  All comparisons are plain IEEE `>`; no multiply
 * appears, so nothing contracts into an FMA; the result is defined for every
 * input, +-inf and NaN rows included.  first_max is breeze's first maximum (the
 * label rule of ldgpu_score, entry 0 of the top-k order): a document of one
 * span gets exactly the label ldgpu_score_spans gives it, an empty document's
 * single empty span gets 0.  With penalty = +inf no span ever switches: a
 * document gets one label throughout.  With penalty = 0 every span may switch
 * for free.
 * Parallelism is one wave per document: a call on a few very long documents
 * is serial in their spans.
 *
 * Host buffers in and out; synchronous and thread-safe as ldgpu_score.
 * out_labels [n_spans], n_spans = span_offsets[n_docs] of ldgpu_span_offsets.
 * Argument checks, LDGPU_EROWLEN, the pipeline over pinned / pageable buffers
 * and the absent document-length limit are those of ldgpu_score_spans.  The
 * pipeline's chunks end at document boundaries (a document's labels are known
 * only after its last span): as many whole documents as fit the span call's
 * span budget and 64 MiB of source bytes, one document at least; a single
 * document beyond the budget is a chunk of its own, cut into span chunks by
 * the device form's loop. */
int ldgpu_score_segments(ldgpu_model* model, const uint8_t* bytes, const int64_t* offsets, int64_t n_docs,
                         int32_t width, int32_t stride, double penalty, int32_t* out_labels /* [n_spans] */);

/* Device-resident variant, asynchronous on `stream` under the rules and
 * argument checks of ldgpu_score_spans_device (d_span_offsets, n_spans and its
 * over-estimate as there: a span index at or beyond d_span_offsets[n_docs]
 * gets label 0), plus the penalty check.  The spans are gathered and scored
 * in chunks as there (each additionally bounded by the top-k call's 256 MiB of
 * scores), every chunk's rows consumed from stream-ordered scratch by the
 * forward pass, with the open document's dp row carried to the next chunk;
 * one backtrace pass follows the last chunk.  Whole-call scratch, also
 * stream-ordered: n_spans * (8 * ceil(n_langs / 64) + 4) bytes of switch words
 * and first-maximum indices, plus two carry rows of n_langs doubles; a failed
 * allocation is LDGPU_ENOMEM and names the size.  Nothing is read back. */
int ldgpu_score_segments_device(ldgpu_model* model, const uint8_t* d_bytes, int64_t n_bytes,
                                const int64_t* d_offsets, int64_t n_docs, int32_t width, int32_t stride,
                                double penalty, const int64_t* d_span_offsets, int64_t n_spans,
                                int32_t* d_labels, void* stream);

/* -------------------------------------------------------------------- FIT */
typedef struct ldgpu_counts ldgpu_counts;

/* A device count table for n_langs languages and the given gram lengths.
 * capacity_hint: expected distinct grams (0 = default); the table grows when
 * it passes half full between batches. */
int ldgpu_counts_create(ldgpu_ctx* ctx, int32_t n_langs, const int32_t* gram_lengths,
                        int32_t n_grams, int64_t capacity_hint, ldgpu_counts** out);
int ldgpu_counts_destroy(ldgpu_counts* counts);
/* The table's language count. */
int ldgpu_counts_langs(const ldgpu_counts* counts, int32_t* n_langs);

/* Accumulate one batch of documents: every window of every gram length is
 * counted for doc_lang[d] (documents whose doc_lang is outside [0, n_langs)
 * are skipped, as reduceGrams filters unsupported languages).  Device
 * scratch per call: the records of up to ~512 MB of corpus at a time (~16 GB,
 * kept by the context for the next call) and a table of the call's maximal
 * windows (one per byte position), from which every gram length's counts are
 * derived before the call returns (FIT v4). */
int ldgpu_count(ldgpu_counts* counts, const uint8_t* bytes, const int64_t* offsets,
                const int32_t* doc_lang, int64_t n_docs);
int ldgpu_count_device(ldgpu_counts* counts, const uint8_t* d_bytes, int64_t n_bytes,
                       const int64_t* d_offsets, const int32_t* d_doc_lang, int64_t n_docs,
                       void* stream);

/* Distinct grams and their total key bytes. */
int ldgpu_counts_size(ldgpu_counts* counts, int64_t* n_grams, int64_t* key_bytes);
/* Distinct grams, distinct (gram, language) pairs -- the rows reduceGrams
 * emits (LanguageDetector.scala:57-65) -- and the sum of all counts (= the
 * windows counted).  Any output pointer may be NULL. */
int ldgpu_counts_stats(ldgpu_counts* counts, int64_t* n_grams, int64_t* n_pairs, int64_t* total);
/* Export sorted by (length, unsigned bytes): key_bytes, key_offsets[n+1],
 * counts[n][n_langs] (raw int64 sums; the JVM sums wrap at 2^31). */
int ldgpu_counts_export(ldgpu_counts* counts, uint8_t* key_bytes, int64_t* key_offsets,
                        int64_t* counts_out);

/* Merge a dense (keys, counts[n][n_langs]) block into the table (used by the
 * multi-GPU merge after an all-reduce over a common key list).  Keys are
 * given packed as in ldgpu_counts_export. */
int ldgpu_counts_add(ldgpu_counts* counts, int64_t n, const uint8_t* key_bytes,
                     const int64_t* key_offsets, const int64_t* counts_in);

/* Sparse form of the table, what crosses a Spark shuffle: the grams
 * [first, first + n) of the (length, bytes) order (0 <= first <= first + n <=
 * n_grams) with their nonzero (language, count) pairs in language order --
 * ~1.3 pairs per gram on the fit corpora against n_langs dense counters.
 * _sparse_size gives the range's key bytes and pairs; _export_sparse writes
 * key_bytes, key_offsets[n + 1] and pair_offsets[n + 1] (both relative to the
 * range), pair_langs and pair_counts.  Exporting in ranges keeps every buffer
 * as small as the caller wants (a JVM direct buffer holds < 2 GiB).
 * _add_sparse adds such a block (keys of 1..15 bytes, counts >= 0). */
int ldgpu_counts_sparse_size(ldgpu_counts* counts, int64_t first, int64_t n, int64_t* key_bytes,
                             int64_t* n_pairs);
int ldgpu_counts_export_sparse(ldgpu_counts* counts, int64_t first, int64_t n, uint8_t* key_bytes,
                               int64_t* key_offsets, int64_t* pair_offsets, int32_t* pair_langs,
                               int64_t* pair_counts);
int ldgpu_counts_add_sparse(ldgpu_counts* counts, int64_t n, const uint8_t* key_bytes,
                            const int64_t* key_offsets, const int64_t* pair_offsets,
                            const int32_t* pair_langs, const int64_t* pair_counts);

/* Device-resident forms of export / add (the multi-GPU merge keeps counts in
 * HBM and exchanges them with RCCL).  Keys are packed u64: bytes little-endian
 * in bits 0..55, length (1..7) in bits 56..63 (a table holding grams of 8..15
 * bytes fails export_device with LDGPU_EUNSUPPORTED: use ldgpu_counts_export).  export_device writes the
 * distinct grams (unordered) into caller buffers of `capacity` entries
 * (keys[capacity], counts[capacity][n_langs] int64) and their number to
 * *n_out; it fails with LDGPU_EINVAL if capacity is too small.  Both are
 * synchronous with respect to `stream` (NULL = HIP's null stream). */
int ldgpu_counts_export_device(ldgpu_counts* counts, int64_t capacity, uint64_t* d_keys,
                               int64_t* d_counts, int64_t* n_out, void* stream);
int ldgpu_counts_add_device(ldgpu_counts* counts, int64_t n, const uint64_t* d_keys,
                            const int64_t* d_counts, void* stream);

/* ------------------------------------------------------- multi-GPU FIT merge
 * Replaces the reference's shuffles of reduceGrams / computeProbabilities /
 * filterTopGrams (LanguageDetector.scala:57-65, :79-81, :110-126) when the
 * corpus is sharded over executors, one GPU each.  A communicator spans the
 * ranks of one fit; two transports run the same merge:
 *   RCCL over xGMI  -- ldgpu_comm_create_rccl; rank 0 makes the id with
 *                      ldgpu_comm_unique_id and the caller hands it to every
 *                      rank (Spark: a driver broadcast);
 *   host callbacks  -- ldgpu_comm_create_host; the caller provides an
 *                      all-gather and an all-to-all over host memory (an
 *                      executor's own transport; gloo in the tests). */
typedef struct ldgpu_comm ldgpu_comm;
#define LDGPU_COMM_ID_BYTES 128

typedef struct {
    void* user;
    /* recv = world * bytes, rank r's block at r * bytes; returns 0 on success */
    int (*allgather)(void* user, const void* send, int64_t bytes, void* recv);
    /* send_bytes[r] bytes to rank r (blocks in rank order), recv_bytes[r]
     * from rank r (blocks in rank order); returns 0 on success */
    int (*alltoallv)(void* user, const void* send, const int64_t* send_bytes, void* recv,
                     const int64_t* recv_bytes);
} ldgpu_host_coll;

int ldgpu_comm_unique_id(uint8_t* out_id /* LDGPU_COMM_ID_BYTES */);
int ldgpu_comm_create_rccl(ldgpu_ctx* ctx, const uint8_t* id, int32_t rank, int32_t world, ldgpu_comm** out);
int ldgpu_comm_create_host(ldgpu_ctx* ctx, int32_t rank, int32_t world, const ldgpu_host_coll* coll,
                           ldgpu_comm** out);
int ldgpu_comm_destroy(ldgpu_comm* comm);

/* Owner-partitioned exchange: gram g belongs to rank owner(g) (a hash of its
 * key), every rank sends its counts of the grams it does not own to their
 * owners (one all-to-all), and afterwards holds the GLOBAL counts (sums over
 * all ranks, bit-exact) of exactly the grams it owns.  ldgpu_counts_export /
 * _size / _stats then describe the owned shard; ldgpu_fit_table_size on the
 * merged table runs the global top-K through the communicator (a (language,
 * class) histogram all-reduce, an all-gather of each rank's tie candidates,
 * an all-gather of the chosen rows), and every rank exports the same table.
 * Grams of 8..15 bytes (their own table) travel by an all-gather of every
 * rank's entries instead, each rank keeping those it owns, and a merged table
 * holding any takes the top-K over every rank's presence rows on the host.
 * Collective: every rank calls it.  Counting more documents into a merged
 * table is an error (LDGPU_EINVAL). */
int ldgpu_counts_merge(ldgpu_counts* counts, ldgpu_comm* comm);

/* computeProbabilities + filterTopGrams: v_l = log(1 + [g in l] / k_g);
 * per language the profile_size largest v_l (ties: ascending (length, bytes));
 * the union of the chosen grams with their full rows.  Two calls: _size
 * computes and caches the table, _export copies it (sorted by (length, bytes)). */
int ldgpu_fit_table_size(ldgpu_counts* counts, int32_t profile_size, int64_t* n_rows,
                         int64_t* key_bytes);
int ldgpu_fit_table_export(ldgpu_counts* counts, uint8_t* key_bytes, int64_t* key_offsets,
                           double* rows);
/* The cached table's rows and key bytes (what the last _size returned);
 * LDGPU_EINVAL before any _size. */
int ldgpu_fit_table_info(ldgpu_counts* counts, int64_t* n_rows, int64_t* key_bytes);
/* The same table in mask form (masks [n_rows][ceil(L/64)], vals [n_rows]):
 * 8 (S + 1) bytes per row instead of 8 L -- what ldgpu_model_create_masks
 * takes (config-5 tables: 10M rows x 200 languages). */
int ldgpu_fit_table_export_masks(ldgpu_counts* counts, uint8_t* key_bytes, int64_t* key_offsets,
                                 uint64_t* masks, double* vals);

/* ----------------------------------------------------------- PREPROCESS */
/* The caller-side preprocessors on the device, over Java strings (UTF-16 code
 * units, offsets in units):
 *   LDGPU_PRE_LOWER  LowerCasePreprocessor (LowerCasePreprocessor.scala:44-76):
 *                    String.toLowerCase(Locale.forLanguageTag(label)) -- each
 *                    unit through the host language's 1:1 mapping (`lower`,
 *                    e.g. Character.toLowerCase), the 1:1 locale rules of
 *                    tr / az (I -> U+0131, U+0130 -> i) applied on the device;
 *   LDGPU_PRE_CLEAN  SpecialCharPreprocessor's documented intent
 *                    (SpecialCharPreprocessor.scala:40-70): the symbols
 *                    / _ [ ] * ( ) % ^ & @ $ # : | { } < > ~ ` " \ and every
 *                    space removed (the reference's own pattern never
 *                    compiles: the JVM throws PatternSyntaxException);
 *   LDGPU_PRE_LOW_BYTES  the output is the SCORE encoding (the low byte of each
 *                    unit, LanguageDetectorModel.scala:226) instead of units:
 *                    ldgpu_score_device's input.
 * A document whose lower-casing is not 1:1 or needs context -- a unit marked
 * in `special` (U+0130 outside tr / az, capital sigma's Final_Sigma rule, the
 * high surrogates of cased supplementary planes), tr / az "I" + U+0307, lt
 * I / J / U+012E before a mark above, U+00CC / U+00CD / U+0128 -- is not
 * processed: host[d] = 1 and its output is empty; the caller lower-cases it
 * itself (the Java locale rules stay on the host). */
#define LDGPU_PRE_LOWER      1
#define LDGPU_PRE_CLEAN      2
#define LDGPU_PRE_LOW_BYTES  4
#define LDGPU_LOCALE_ROOT    0  /* per-document locale class of the label */
#define LDGPU_LOCALE_TR_AZ   1  /* Locale.forLanguageTag(label).getLanguage() is tr or az */
#define LDGPU_LOCALE_LT      2  /* ... lt */

typedef struct ldgpu_casemap ldgpu_casemap;
/* lower: [65536] the lower-case unit of each unit (1:1); special: [8192]
 * bytes, bit u set = unit u sends its document to the host. */
int ldgpu_casemap_create(ldgpu_ctx* ctx, const uint16_t* lower, const uint8_t* special, ldgpu_casemap** out);
int ldgpu_casemap_destroy(ldgpu_casemap* map);
/* Device buffers, asynchronous on `stream` (NULL: the default stream).
 * d_out holds up to d_offsets[n_docs] - d_offsets[0] units (bytes with
 * LDGPU_PRE_LOW_BYTES); d_out_offsets [n_docs + 1] receives the output's
 * offsets (from 0); d_host [n_docs]; d_locale (nullable: root) [n_docs]. */
int ldgpu_preprocess_device(ldgpu_casemap* map, const uint16_t* d_units, const int64_t* d_offsets,
                            int64_t n_docs, const uint8_t* d_locale, int32_t flags, void* d_out,
                            int64_t* d_out_offsets, uint8_t* d_host, void* stream);
/* The same over host buffers (copied in and out; returns when done). */
int ldgpu_preprocess(ldgpu_casemap* map, const uint16_t* units, const int64_t* offsets, int64_t n_docs,
                     const uint8_t* locale, int32_t flags, void* out, int64_t* out_offsets, uint8_t* host);

/* ---------------------------------------------------------------- UTF-8 */
/* FIT counts a text's UTF-8 bytes, SCORE scans the low byte of every UTF-16
 * code unit (LanguageDetector.scala:37, LanguageDetectorModel.scala:161).  These
 * calls take the UTF-8 a caller stores and produce the other side's input on
 * the device: UTF-16 units (ldgpu_preprocess_device's input) or, with
 * LDGPU_PRE_LOW_BYTES, the SCORE encoding (ldgpu_score_device's input).
 *
 * A document is well-formed iff its bytes are a concatenation of the sequences
 * of Unicode Table 3-7:
 *   00..7F
 *   C2..DF 80..BF
 *   E0     A0..BF 80..BF
 *   E1..EC 80..BF 80..BF
 *   ED     80..9F 80..BF
 *   EE..EF 80..BF 80..BF
 *   F0     90..BF 80..BF 80..BF
 *   F1..F3 80..BF 80..BF 80..BF
 *   F4     80..8F 80..BF 80..BF
 * Everything else is ill-formed: C0, C1 and F5..FF anywhere, a continuation
 * byte without a lead, an overlong form, an encoded surrogate (ED A0..BF), a
 * value beyond U+10FFFF, and a sequence cut off by the end of its document (a
 * sequence never borrows bytes from the next document).  These are exactly the
 * byte strings CPython's bytes.decode("utf-8") accepts.  00 is an ordinary
 * character (C0 80 is ill-formed); EF BB BF is U+FEFF and stays in the output.
 *
 * Units of a well-formed document: a code point cp < 0x10000 gives the unit
 * cp; a larger one, v = cp - 0x10000, the two units 0xD800 + (v >> 10) and
 * 0xDC00 + (v & 0x3FF) -- what new String(bytes, UTF_8) and
 * UTF8String.toString give, so an output index is a Java String index.  With
 * LDGPU_PRE_LOW_BYTES the output is (uint8_t)unit per unit.
 *
 * An ill-formed document is not decoded: host[d] = 1 and its output is empty
 * (out_offsets[d + 1] == out_offsets[d]).  Which replacement characters a
 * decoder would insert stays the caller's business, as the context-dependent
 * documents of the preprocessors do. */
#define LDGPU_UTF8_STEP_BYTES 256  /* bytes of a document one wave takes per step (tests place sequences across it) */

/* Device buffers, asynchronous on `stream` (NULL: the default stream).  flags:
 * 0 or LDGPU_PRE_LOW_BYTES, anything else is LDGPU_EINVAL.  d_utf8 must be
 * 4-byte aligned, and the bytes up to d_offsets[n_docs] rounded up to 4 must
 * be readable (the rule of ldgpu_score_device's d_bytes); nothing beyond them
 * and nothing before d_offsets[0] rounded down to 4 is read.  d_out holds
 * d_offsets[n_docs] - d_offsets[0] units (bytes with the flag): a document
 * never gives more units than it has bytes.  d_out_offsets [n_docs + 1]
 * receives the output's offsets (from 0); d_host [n_docs].  Offsets are
 * trusted; n_docs < 2^31 - 1 (the scan), beyond is LDGPU_EUNSUPPORTED. */
int ldgpu_utf8_decode_device(ldgpu_ctx* ctx, const uint8_t* d_utf8, const int64_t* d_offsets, int64_t n_docs,
                             int32_t flags, void* d_out, int64_t* d_out_offsets, uint8_t* d_host, void* stream);
/* The same over host buffers (copied in and out; returns when done). */
int ldgpu_utf8_decode(ldgpu_ctx* ctx, const uint8_t* utf8, const int64_t* offsets, int64_t n_docs,
                      int32_t flags, void* out, int64_t* out_offsets, uint8_t* host);

/* ldgpu_score on UTF-8 documents.  A well-formed document's label and score
 * row are bit for bit those ldgpu_score gives for its SCORE encoding, on every
 * model layout.  An ill-formed document gets label -1 and the score row of an
 * empty document: the caller decodes it under its own replacement rule and
 * scores it with ldgpu_score.  Only the UTF-8 bytes cross to the device; each
 * chunk is decoded there and scored from the decoded bytes.  Argument checks,
 * LDGPU_EROWLEN, thread safety and the pipeline over pinned / pageable buffers
 * are those of ldgpu_score; the 2^28 limit applies to a document's UTF-8
 * length. */
int ldgpu_score_utf8(ldgpu_model* model, const uint8_t* utf8, const int64_t* offsets, int64_t n_docs,
                     int32_t* out_labels, double* out_scores);
/* Device-resident variant, asynchronous on `stream` under the rules of
 * ldgpu_score_device (d_utf8 4-byte aligned, n_bytes >= d_offsets[n_docs]).
 * The documents are decoded into stream-ordered scratch (n_bytes of decoded
 * bytes, the offsets and flags of a chunk of at most 2^24 documents) and scored
 * from there: nothing is read back. */
int ldgpu_score_utf8_device(ldgpu_model* model, const uint8_t* d_utf8, int64_t n_bytes, const int64_t* d_offsets,
                            int64_t n_docs, int32_t* d_labels, double* d_scores, void* stream);

/* ------------------------------------------- UTF-8: top-k, spans, segments */
/* The top-k, span and segment forms of SCORE on UTF-8 documents, and every
 * span's start as a byte position in its UTF-8 document.  (The names end in
 * _utf.)  The rule:
 *   - width and stride count UTF-16 units (= SCORE bytes), exactly as in
 *     ldgpu_score_spans.
 *   - A document's spans are those of ldgpu_span_offsets applied to its unit
 *     count u: one span if u <= width, otherwise 1 + ceil((u - width) / stride).
 *   - Well-formedness is ldgpu_utf8_decode's rule (Unicode Table 3-7).  An
 *     ill-formed document counts as u = 0: it has one empty span.
 *   - units[d] is u for a well-formed document and -1 for an ill-formed one.
 *   - start[i], for span j of document d, is an int64 byte index relative to
 *     the document's first byte: the index of the lead byte of the character
 *     that unit j * stride belongs to.  If unit j * stride is the low surrogate
 *     of a 4-byte character (the boundary splits the pair), it is that
 *     character's lead byte.  A character's bytes therefore always belong to
 *     one run, the one starting at or before its first unit.  At stride == 1
 *     both units of a pair give the same start.  Span 0 of every document has
 *     start 0; this includes an empty document's single span and an ill-formed
 *     document's single span.  Starts are non-decreasing within a document.
 *     Every start is < len for a non-empty well-formed document.
 *   - Labels and score rows of a well-formed document's spans are bit for bit
 *     those of ldgpu_score_spans, ldgpu_score_segments or ldgpu_score_topk on
 *     its SCORE encoding, on every model layout.
 *   - For an ill-formed document: its single span gets label -1 and the empty
 *     document's score row; the top-k form gives -1 in all k label entries and
 *     0.0 in the scores; the segment form gives -1.
 *   - Byte runs (languagedetection.utf8.byte_runs) turn span labels into runs
 *     in bytes.  Span j owns bytes [start[j], start[j+1]), the last span up to
 *     the document's byte length.  Consecutive spans of one label merge.  Empty
 *     runs are dropped.  This is the byte twin of languagedetection.spans.runs.
 *
 * Span offsets.  The span count depends on the unit count, which only a decode
 * knows, so the span offsets come from the device: the device form runs the
 * decoder's length pass and the span-offset arithmetic on the unit counts and
 * reads nothing back (asynchronous on `stream`; d_utf8 4-byte aligned, offsets
 * trusted, n_docs < 2^31 - 1 as in ldgpu_utf8_decode_device; d_units nullable).
 * The host form copies the UTF-8 in, runs the device form and copies
 * 8 (n_docs + 1) (+ 8 n_docs) bytes back; the offsets are checked as by
 * ldgpu_score.  On the host route the UTF-8 therefore crosses PCIe twice: once
 * here and once in the scoring call. */
int ldgpu_span_offsets_utf(ldgpu_ctx* ctx, const uint8_t* utf8, const int64_t* offsets, int64_t n_docs,
                           int32_t width, int32_t stride, int64_t* span_offsets /* [n_docs + 1] */,
                           int64_t* units /* [n_docs], nullable */);
int ldgpu_span_offsets_utf_device(ldgpu_ctx* ctx, const uint8_t* d_utf8, const int64_t* d_offsets, int64_t n_docs,
                                  int32_t width, int32_t stride, int64_t* d_span_offsets,
                                  int64_t* d_units /* nullable */, void* stream);

/* ldgpu_score_topk on UTF-8 documents.  Argument checks, LDGPU_EROWLEN, thread
 * safety and the pipeline are those of ldgpu_score_topk; the 2^28 limit applies
 * to a document's UTF-8 length.  Each chunk is decoded on the device and
 * scored and selected from the decoded bytes. */
int ldgpu_score_topk_utf(ldgpu_model* model, const uint8_t* utf8, const int64_t* offsets, int64_t n_docs,
                         int32_t k, int32_t* out_top_labels, double* out_top_scores /* nullable */);
/* Device-resident variant, asynchronous on `stream` under the rules of
 * ldgpu_score_utf8_device: d_utf8 4-byte aligned, n_bytes >= d_offsets[n_docs],
 * offsets trusted.  The call decodes into stream-ordered scratch: n_bytes of
 * low bytes, plus the offsets and flags of all n_docs documents;
 * n_docs >= 2^31 - 1 is LDGPU_EUNSUPPORTED.  Nothing is read back. */
int ldgpu_score_topk_utf_device(ldgpu_model* model, const uint8_t* d_utf8, int64_t n_bytes,
                                const int64_t* d_offsets, int64_t n_docs, int32_t k, int32_t* d_top_labels,
                                double* d_top_scores, void* stream);

/* ldgpu_score_spans on UTF-8 documents.  span_offsets [n_docs + 1] is the
 * output of the span-offset call above for the same width and stride; it is
 * checked (NULL, a first entry other than 0, a decrease, a document without a
 * span: LDGPU_EINVAL).  out_labels [n_spans], out_scores nullable
 * [n_spans][n_langs], out_starts nullable [n_spans] (the starts of the rule
 * above), n_spans = span_offsets[n_docs].  Argument checks, LDGPU_EROWLEN,
 * thread safety and the absent document-length limit are those of
 * ldgpu_score_spans.  The pipeline's chunks end at document boundaries, cut as
 * ldgpu_score_segments cuts them: whole documents within the span budget (with
 * scores also the top-k call's 256 MiB of score rows) and 64 MiB of UTF-8
 * bytes, one at least; the chunk is decoded on the device and its spans are
 * gathered and scored from the decoded bytes in span chunks. */
int ldgpu_score_spans_utf(ldgpu_model* model, const uint8_t* utf8, const int64_t* offsets, int64_t n_docs,
                          int32_t width, int32_t stride, const int64_t* span_offsets, int32_t* out_labels,
                          double* out_scores /* nullable */, int64_t* out_starts /* nullable */);
/* Device-resident variant, asynchronous on `stream` under the rules of the
 * top-k variant above (alignment, scratch, the n_docs limit) and of
 * ldgpu_score_spans_device: n_spans may over-estimate d_span_offsets[n_docs];
 * an index at or beyond it gets label 0 and start 0.  With d_starts NULL no
 * start is computed. */
int ldgpu_score_spans_utf_device(ldgpu_model* model, const uint8_t* d_utf8, int64_t n_bytes,
                                 const int64_t* d_offsets, int64_t n_docs, int32_t width, int32_t stride,
                                 const int64_t* d_span_offsets, int64_t n_spans, int32_t* d_labels,
                                 double* d_scores /* nullable */, int64_t* d_starts /* nullable */, void* stream);

/* ldgpu_score_segments on UTF-8 documents: span_offsets, out_starts, checks and
 * chunks as in the span form above, the penalty check of
 * ldgpu_score_segments. */
int ldgpu_score_segments_utf(ldgpu_model* model, const uint8_t* utf8, const int64_t* offsets, int64_t n_docs,
                             int32_t width, int32_t stride, double penalty, const int64_t* span_offsets,
                             int32_t* out_labels, int64_t* out_starts /* nullable */);
int ldgpu_score_segments_utf_device(ldgpu_model* model, const uint8_t* d_utf8, int64_t n_bytes,
                                    const int64_t* d_offsets, int64_t n_docs, int32_t width, int32_t stride,
                                    double penalty, const int64_t* d_span_offsets, int64_t n_spans,
                                    int32_t* d_labels, int64_t* d_starts /* nullable */, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LDGPU_H */
