/*
 * kgx.h -- C ABI of the MI355X-native close_kmers hot path:
 *          k-mer encode -> signature-hash probe -> hit-run scoring.
 *
 * The reference runs this path as KmerGuts::process_aa_seq over a memory-mapped
 * KmerImage, one KmerGuts per CPU pool thread (threadpool.cc:18-44).  This ABI
 * replaces that per-sequence C++ call with batched entry points over plain
 * pointers and sizes (no C++ or torch types), implemented by hand-written
 * gfx950 HIP kernels (close_kmers_amd/csrc/).  The C++ facade in
 * close_kmers_amd/csrc/kguts_hip.h re-exposes the KmerGuts surface on top of
 * it; INTEGRATION.md shows the bindings.
 *
 * Error behaviour: every entry point returns KGX_OK (0) or a negative KGX_E*
 * code and never exits (the reference exit()s on bad files,
 * kmer_image.cc:88-147, kguts.cc:550-552).  kgx_last_error() returns a
 * thread-local message for the last failure.
 *
 * Threading: a kgx_image is read-only after creation and may be shared by any
 * number of contexts; a kgx_ctx is NOT thread-safe, exactly like KmerGuts
 * (kguts.h:263-266) -- create one per host worker thread (threadpool.h:42).
 */
#ifndef KGX_H
#define KGX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ----------------------------------------------------- */
#define KGX_OK 0
#define KGX_EINVAL (-1)   /* bad argument */
#define KGX_EIO (-2)      /* cannot open / read a file */
#define KGX_EFORMAT (-3)  /* image size / version / entry size mismatch */
#define KGX_ENOMEM (-4)   /* host or device allocation failed */
#define KGX_EDEVICE (-5)  /* HIP runtime error or no gfx950 device */
#define KGX_ERANGE (-6)   /* image or batch larger than supported */
#define KGX_EFULL (-7)    /* image builder: table would reach half full */
#define KGX_EBUSY (-8)    /* call service: no free slot, or not a call it serves (use a batch path) */

/* ---- what kgx_process_* computes --------------------------------------- */
#define KGX_WANT_HITS 1u  /* hit list (what hit_cb receives, kguts.cc:814-815) */
#define KGX_WANT_CALLS 2u /* KmerCall runs (process_set_of_hits, kguts.cc:734-781) */
#define KGX_WANT_OTU 4u   /* OTU tallies (KmerOtuStats, kguts.h:185-219), on the device */
#define KGX_WANT_BEST 8u  /* find_best_call per sequence, on the device (kgx_best_call) */

/* ---- on-disk / in-HBM record layouts (kmer_image.h:11-23) -------------- */
typedef struct kgx_image_header { /* kmer_memory_image_t */
    uint64_t num_sigs;            /* buckets */
    uint64_t entry_size;          /* 24 */
    int64_t version;              /* 1 (KMER_VERSION, kmer_image.h:6) */
} kgx_image_header;

typedef struct kgx_sig_kmer { /* sig_kmer_t: one 24-byte bucket */
    uint64_t which_kmer;      /* > 20^8 means empty (kguts.cc:106-107) */
    int32_t otu_index;
    uint16_t avg_from_end;
    uint16_t pad;
    int32_t function_index;
    float function_wt;
} kgx_sig_kmer;

/* One hit: KmerGuts::hit_in_sequence_t (kguts.h:228-233) = the bucket copy +
 * the window offset, plus the sequence index within the batch.  32 bytes. */
typedef struct kgx_hit {
    uint64_t which_kmer;
    int32_t otu_index;
    uint16_t avg_from_end;
    uint16_t flags; /* KGX_HIT_* (the bucket's pad bytes in the reference) */
    int32_t function_index;
    float function_wt;
    uint32_t pos; /* offset of the 8-mer in the protein (pLoc, kguts.cc:803) */
    uint32_t seq; /* index of the sequence in the batch */
} kgx_hit;
/* hit flags are set only when KGX_WANT_OTU is requested (they feed the OTU
 * tally); otherwise they are 0 */
#define KGX_HIT_IN_RUN 1u /* appended to the run buffer (kguts.cc:845-851) */
#define KGX_HIT_OTU 2u    /* tallied into otu_map by an emitted call (kguts.cc:760-768) */
#define KGX_HIT_COUNTED 4u /* buffered while its function was the run's current_fI */

/* KmerCall (kguts.h:166-183), 20 bytes */
typedef struct kgx_call {
    uint32_t start;
    uint32_t end;
    int32_t count;
    uint32_t function_index;
    float weighted_hits;
} kgx_call;

/* What find_best_call (kguts.cc:1008-1199) decides for one sequence's calls,
 * computed on the device.  The function names stay on the host:
 *   kind 0  no calls: function_index -1, function "", score 0, weighted 0,
 *           score_offset left as the caller had it (kguts.cc:1015-1018)
 *   kind 1  called: function_index fi0, function = name(fi0)
 *   kind 2  ambiguous pair: function_index -1, function = the lexically
 *           larger of name(fi0), name(fi1) + " ?? " + the other
 *   kind 3  no call: function_index -1, function "", score_offset written
 * score / weighted_score / score_offset are the reference's values in every
 * kind (fi0 / fi1 are the top two functions whenever there are two). */
typedef struct kgx_best_call {
    int32_t kind;
    int32_t fi0;
    int32_t fi1;
    float score;
    float weighted_score;
    float score_offset;
} kgx_best_call;

/* one (otu_index, count) pair of KmerOtuStats::otus_by_count (kguts.h:214-218) */
typedef struct kgx_otu {
    int32_t otu_index;
    int32_t count;
} kgx_otu;

/* KmerGuts parameters (kguts.cc:236-268); kgx_params_default() gives
 * min_hits=5, max_gap=200, order_constraint=0, min_weighted_hits=0.
 * min_hits <= 0 makes the reference read hits[-2] at the final flush (UB);
 * here such a flush emits nothing. */
typedef struct kgx_params {
    int32_t min_hits;
    int32_t max_gap;
    int32_t order_constraint;
    int32_t min_weighted_hits;
} kgx_params;

/* Host views of a batch's results (CSR by sequence).  Owned by the context
 * and valid until the next call on it.  otus are in otus_by_count order. */
typedef struct kgx_result {
    uint32_t n_seq;
    const uint64_t *hit_offsets; /* n_seq + 1 */
    const kgx_hit *hits;
    const uint64_t *call_offsets; /* n_seq + 1 */
    const kgx_call *calls;
    const uint64_t *otu_offsets; /* n_seq + 1 */
    const kgx_otu *otus;
    uint64_t n_windows; /* window positions, sum of max(0, len-8); those holding a
                           non-standard residue are skipped, not probed */
    const kgx_best_call *best; /* n_seq entries with KGX_WANT_BEST, else NULL */
} kgx_result;

/* Device-resident results of kgx_run_device (pointers into HBM).
 * Windows are numbered across the batch: sequence s owns global windows
 * [window_base[s], window_base[s+1]) (position = global - window_base[s]).
 * The probe works in tiles of tile_windows consecutive windows; tile t's hits
 * are stored compacted in window order from slot t * tile_windows, and bit i
 * of hit_mask[g] is set when global window 64*g + i hit.  So the hits of a
 * sequence are, word by word of its mask range, contiguous stretches of its
 * tiles' hit lists, and a hit's window (hence its sequence and position)
 * is its mask bit.  Hit records, by hit_format:
 *   KGX_HIT_PACKED16 (PACKED16 images): one 16-byte record per slot in
 *     hits_hot, the matching table record itself (kgx_image_set_layout's
 *     packed layout), flags (KGX_HIT_*) in bits 28-30 of its 4th word;
 *     hits_cold is NULL;
 *   KGX_HIT_PLANES (AOS24 images): two 16-byte records at the same slot:
 *     hits_hot[i]  = {avg_from_end | flags << 16, function_index, function_wt, pos}
 *     hits_cold[i] = {which_kmer (low, high 32 bits), otu_index, seq}
 * Calls of s are contiguous from calls[window_base[s]]; counts are
 * hit_count[s] / call_count[s]. */
typedef struct kgx_device_result {
    uint32_t n_seq;
    uint32_t tile_windows;
    const uint64_t *window_base; /* n_seq + 1: exclusive scan of max(0, len-8) */
    const uint64_t *hit_mask;    /* ceil(window_base[n_seq] / 64) words */
    const uint32_t *hit_count;   /* n_seq */
    const uint32_t *call_count;  /* n_seq */
    const uint32_t *hits_hot;    /* 4 words per slot, capacity window_base[n_seq] slots */
    const uint32_t *hits_cold;   /* 4 words per slot */
    const kgx_call *calls;       /* capacity window_base[n_seq] */
    const kgx_best_call *best;   /* n_seq, after a score stage with KGX_WANT_BEST, else NULL */
    uint32_t hit_format;         /* KGX_HIT_PACKED16 or KGX_HIT_PLANES */
    /* with KGX_WANT_OTU (else NULL): sequence s's KmerOtuStats::otus_by_count
     * pairs at otus[window_base[s] ..+ otu_count[s]) */
    const uint32_t *otu_count;   /* n_seq */
    const kgx_otu *otus;
} kgx_device_result;
#define KGX_HIT_PLANES 0u
#define KGX_HIT_PACKED16 1u

typedef struct kgx_image kgx_image;
typedef struct kgx_ctx kgx_ctx;

/* ---- library ------------------------------------------------------------ */
const char *kgx_version(void);
const char *kgx_last_error(void);
const char *kgx_strerror(int code);
/* number of visible gfx950 devices (0 in a GPU-less container) */
int kgx_device_count(void);
int kgx_params_default(kgx_params *p);
/* How the library's host threads wait for their own device work (the small-
 * batch path, rollups, collects): KGX_WAIT_SPIN (the default: the HIP
 * runtime's own wait, which polls), KGX_WAIT_SLEEP (poll every poll_us, the
 * thread asleep in between; poll_us 0 = 20) or KGX_WAIT_BLOCK (blocking-sync
 * events).  Process-wide; the environment variable KGX_HOST_WAIT
 * (spin|sleep[:us]|block) sets the starting mode.  A server whose workers
 * share a CPU quota gives the spinning time back to its other threads. */
#define KGX_WAIT_SPIN 0
#define KGX_WAIT_SLEEP 1
#define KGX_WAIT_BLOCK 2
int kgx_set_host_wait(int mode, uint32_t poll_us);
int kgx_get_host_wait(uint32_t *poll_us);
/* set_parameters (kguts.cc:244-268) over parallel name/value string arrays:
 * resets to the defaults, then applies std::stoi to the four known names;
 * an unparsable value leaves the default (the reference only warns). */
int kgx_params_parse(kgx_params *p, const char *const *names, const char *const *values, size_t n);

/* ---- images: replaces KmerImage (kmer_image.h:25-39, kmer_image.cc) ----- */
/* Load <dir>/kmer.table.mem_map into HBM of `device`, validating size,
 * version and entry size exactly as kmer_image.cc:128-147. */
int kgx_image_open(const char *dir, int device, kgx_image **out);
/* One replica per entry of devices[0..n) (north_star: the read-only image
 * replicated per GPU): the file is read ONCE -- each chunk is pread into
 * pinned host memory and copied up to every device on that device's own
 * link -- then every replica is packed on its device.  A device may be
 * listed more than once (independent replicas on one GPU).  out[i] receives
 * the replica on devices[i]; on failure every out[i] is NULL.  Replaces one
 * KmerImage per process (threadpool.cc:18-20) when a process drives several
 * GPUs. */
int kgx_image_open_replicas(const char *dir, const int *devices, uint32_t n, kgx_image **out);
/* A replica of src on `device`, copied device to device (hipMemcpyPeer: over
 * xGMI between two GPUs, a local copy on the same GPU): same resident layout
 * and presence filter, identical lookups. */
int kgx_image_replicate(const kgx_image *src, int device, kgx_image **out);
/* Same, from an in-memory file image (header followed by the table). */
int kgx_image_from_memory(const void *file_bytes, uint64_t nbytes, int device, kgx_image **out);
/* Synthetic image built in HBM (close_kmers_amd/synth.py documents the
 * generator): n_keys entries in num_sigs buckets, duplicates dropped (lowest
 * entry id wins), linear probing as kguts.cc:166-171.  *n_stored receives the
 * number of distinct keys stored. */
int kgx_image_build_synthetic(uint64_t n_keys, uint64_t num_sigs, int device, kgx_image **out,
                              uint64_t *n_stored);
/* The same generator (source proteins of the n_keys spec), its entry stream
 * extended past n_keys with random keys, cut after the first *n_entries
 * entries that hold exactly n_distinct distinct keys (the smallest such
 * count): SURVEY §8(d)'s "1B-entry image" = 1e9 distinct keys stored. */
int kgx_image_build_synthetic_distinct(uint64_t n_keys, uint64_t n_distinct, uint64_t num_sigs, int device,
                                       kgx_image **out, uint64_t *n_entries);
/* An image from caller entries (host arrays, n each), in num_sigs buckets:
 * KmerGuts::insert_kmer semantics (kguts.cc:166-228) -- keys above 20^8
 * are skipped, KGX_EFULL when the valid entries (duplicates included) reach
 * num_sigs / 2; of duplicated keys the lowest index is the one lookups find,
 * as with the sequential builder.  Distinct keys land in the buckets a
 * sequential build in index order gives them (the table is, byte for byte,
 * what save_kmer_hash_table writes); a duplicated key is stored once, where
 * the sequential builder also stores its later copies. */
int kgx_image_build(const uint64_t *keys, const int32_t *function_index, const int32_t *otu_index,
                    const uint16_t *avg_from_end, const float *function_wt, uint64_t n, uint64_t num_sigs,
                    int device, kgx_image **out, uint64_t *n_stored);
/* write <dir>/kmer.table.mem_map in the file format (save_kmer_hash_table,
 * kguts.cc:194-234 with the header of kmer_image.h:25-30), loadable by
 * KmerImage and kgx_image_open */
int kgx_image_save(const kgx_image *img, const char *dir);
int kgx_image_close(kgx_image *img);
uint64_t kgx_image_num_sigs(const kgx_image *img);
int kgx_image_device(const kgx_image *img);
/* HBM-resident layouts.  The file format is never changed; in HBM an image
 * is kept either as the file's 24-byte buckets (AOS24) or, when every stored
 * bucket has function_index in [-1, 2^20-2] and otu_index in [-1, 2^21-2],
 * as one 16-byte record per bucket at the same slot (PACKED16: one aligned
 * load per bucket examined; 2/3 of the memory).  Lookups give identical
 * results in both.  Images are packed at load when they fit. */
enum { KGX_LAYOUT_AOS24 = 0, KGX_LAYOUT_PACKED16 = 1 };
int kgx_image_layout(const kgx_image *img);
/* convert the resident table in place; KGX_ERANGE if PACKED16 is asked for
 * an image whose payloads do not fit (the image is left unchanged) */
int kgx_image_set_layout(kgx_image *img, int layout);
/* Line index of a PACKED16 image: the same records again in 64-B lines of 4
 * buckets, each key's home at the start of its home line, n_lines = stored
 * keys * 64 / keys_per_64_lines (0 drops the index).  The home line is chosen
 * by the environment variable KGX_LINE_HOME, read at each call (anything but
 * unset, "", "0" or "1" is KGX_EINVAL) and kept with the index it builds:
 *   0            key mod n_lines;
 *   1 (default)  the minimizer home: of the key's two overlapping 7-mers (its
 *                first and its last seven residues) the one with the smaller
 *                hash is hashed to the line, so two neighbouring windows of a
 *                sequence share a line one time in three and the wave that
 *                probes them asks for it once (0.71 random 64-B requests per
 *                window instead of 1.02), at the price of lumpier lines (3%
 *                of the stored keys leave their first line instead of 0.01%).  Built from every
 * bucket the reference's probe (lookup_hash_entry, kguts.cc:585-602) reaches
 * first for its key -- a duplicate further on, or an entry behind a stop
 * bucket, is never found there and is left out -- so every probe (batches,
 * fq, the call service) returns exactly what it returns over the reference
 * slots, while a key's chain nearly always ends in its first line: one random
 * 64-B request per window instead of ~1.05.  Costs 64 B * n_lines of HBM
 * beside the PACKED16 table, which downloads, saves and filters keep using.
 * Like set_layout, no call may run on the image meanwhile.  Replicas
 * (kgx_image_replicate) do not inherit it: build it on each that should.
 * Loads past ~48 (75% of the buckets) are accepted for tests of full lines,
 * but linear probing there walks ~1/(1-a)^2 buckets per miss: the build's
 * insert walks and the probes' chains grow steeply (results stay exact);
 * 36 is the measured load.
 * The index also carries overflow marks: 16 spare bits per line (bits 60-63
 * of each record's second word, which PACKED16 leaves 0) say which of 16
 * hash classes of keys were pushed on past that full line when the index was
 * built.  The line probe ends an absent key's chain at the first full line
 * whose mark for it is clear instead of walking on to an empty bucket; hit
 * records leave every probe with those bits cleared.  The environment
 * variable KGX_LINE_MARKS, read at each call like KGX_LINE_HOME, turns them
 * off: 1 builds marks (the default), 0 builds none; any other value is
 * KGX_EINVAL and the index the image had is kept.  Which bits are set depends
 * on the build's insertion order and differs from build to build; results do
 * not.
 * Twin records.  Under the minimizer home with marks, and at loads up to
 * KGX_LINE_TWINS_MAX_LOAD, every key whose two 7-mers are homed on different
 * lines is stored twice, once from each home, in the same n_lines (at load 36
 * the records fill 28% of the buckets instead of 14%).  The batch line probe
 * then starts a window with an even index in its batch at the home of its
 * last seven residues and an odd one at the home of its first seven: the two
 * windows of such a pair in one sequence always ask for the same line, half a
 * line per window at best where the minimizer alone gives two thirds.  Every
 * other prober keeps starting at the minimizer home and finds what it found.
 * The environment variable KGX_LINE_TWINS, read at each call like the two
 * above: 1 (the default) builds twins where this rule allows, 0 builds none
 * (the index of the paragraphs above, unchanged); any other value is
 * KGX_EINVAL and the index the image had is kept.  The cut is where the
 * doubled records fill half of the buckets.  tools/line_home_model.py
 * (--load), requests per window of a benchmark-shaped batch with twins
 * against without: load 36 0.554 / 0.697, 48 0.585 / 0.700, 64 0.663 / 0.706,
 * 80 0.847 / 0.714, 96 1.448 / 0.726 (full lines with twins: 12%, 19%, 31%,
 * 44%, 61%).  Twins pay up to load 64 and cost past it; at load 255 the
 * doubled records would not fit at all.  The price at every load is paid by
 * the probers that start at the minimizer home: their chains cross the fuller
 * lines (the call service's p50 is a quarter longer at load 36, DESIGN.md
 * section 5); KGX_LINE_TWINS=0 is for images that serve those.
 * Pairs.  Where twins are built and the index has at least 3 lines, a 7-mer
 * can own an aligned 128-byte block, lines 2k and 2k + 1, instead of one line:
 * the keys that end in it are homed on line 2k and the keys that begin with it
 * on line 2k + 1.  Every stored key then has two records (its two homes differ
 * in parity), a line collects at most 20 keys where it collected 40, and the
 * two windows of a pair start on the two halves of one block, which the batch
 * line probe reads by neighbouring quads of one instruction: one 128-byte
 * request.  n_lines and the memory are unchanged; with n_lines odd the last
 * line is nobody's home and chains wrap through it as before.  Every other
 * prober starts at the home of the lower-hashing 7-mer in its role.  The
 * environment variable KGX_LINE_PAIRS, read at each call like the three above:
 * 1 builds pairs wherever this rule allows, 0 builds none, any other value is
 * KGX_EINVAL with the index the image had kept; unset, pairs are built only
 * for an index of more than KGX_LINE_PAIRS_MIN_LINES lines (256 MiB).  Small
 * indexes keep the layout of the paragraphs above because the tests that
 * restate its twin count and homes in Python are written for that layout and
 * build small indexes; the layout pays only where the table is far larger than
 * the caches anyway. */
#define KGX_LINE_TWINS_MAX_LOAD 64u
#define KGX_LINE_PAIRS_MIN_LINES (1ull << 22)
int kgx_image_set_line_index(kgx_image *img, uint32_t keys_per_64_lines);
/* lines of the image's line index (0: none) */
uint64_t kgx_image_line_count(const kgx_image *img);
/* the KGX_LINE_HOME mode the image's line index was built with (0: mod or
 * no index, 1: minimizer) */
uint32_t kgx_image_line_home(const kgx_image *img);
/* twin records in the image's line index: the keys with two distinct home
 * lines, under pairs every stored key (0: built without twins, or no index) */
uint64_t kgx_image_line_twins(const kgx_image *img);
/* 1 when the image's line index was built with pairs (KGX_LINE_PAIRS), else 0 */
uint32_t kgx_image_line_pairs(const kgx_image *img);
/* A device pass over the line index: out[0] stored keys (a key with a twin
 * record counts once), [1] records past their home line (with twins: pairs of
 * a key and one of its home lines where that line does not hold the key), [2] full lines, [3] lines with any overflow mark, [4] mark
 * bits set, [5] missing marks (a stored key lies past a line whose bit for it
 * is clear; 0 for an index with marks, else probes would miss stored keys),
 * [6] unjustified marks (a set bit that no stored key past that line calls
 * for; 0, or the marks would end fewer chains than they can), [7] reserved,
 * 0.  An index built with KGX_LINE_MARKS=0 has [3] = [4] = [6] = 0 and [5]
 * the marks it would carry.  The marks called for are recomputed by the walk
 * that set them (from each displaced record's home line to the line before
 * its own; with twins, from each home of a key to the line before the first
 * that holds it), so [5] = [6] = 0 says that the index holds exactly that walk's
 * marks and no stray bit; that the walk itself is the right one is what the
 * comparisons with the reference's results check.  KGX_EINVAL without a line
 * index; needs 2 B per line of device memory while it runs. */
int kgx_image_line_stats(const kgx_image *img, uint64_t out[8]);
/* Presence filter: 2^log2_bits bits (0 removes it), two bits per stored key
 * in one 64-bit word (blocked Bloom filter).  A probe whose key misses the
 * filter skips the table -- exactly the miss it would have found -- so
 * results never change; a filter small enough to stay in the 256 MiB
 * Infinity Cache turns most misses' DRAM reads into cache reads.  It
 * depends on the key set only (layout changes keep it); contexts use it
 * unless "probe_filter" is 0. */
int kgx_image_set_filter(kgx_image *img, int log2_bits);
/* device pointer to the num_sigs * 24-byte table; NULL while PACKED16 */
const void *kgx_image_table(const kgx_image *img);
/* copy the table as the file's num_sigs * 24-byte buckets to host memory
 * (from PACKED16: pad fields read 0; buckets with a key above 20^8 read as
 * {20^8+1, 0, 0, 0, 0, 0.0}) */
int kgx_image_download(const kgx_image *img, void *dst, uint64_t nbytes);

/* ---- signature selection: build_signature_kmers.cc on the device --------- */
/* From function-labelled proteins to the entries of an image (DESIGN.md
 * §8.8 states the rules): every window of 8 letters out of the 40 of
 * ACDEFGHIKLMNPQRSTVWY / acdefghiklmnpqrstvwy in a sequence whose
 * seq_function is >= 0 gives a tuple; a set = the tuples of one raw 8-byte
 * key (upper and lower case differ); a set is kept when its most frequent
 * function holds at least 80% of it (process_set's float test).  A kept
 * set's record carries that function, the median of its tuples' distances
 * from the end of their sequences, and compute_weight_of_signature's weight.
 * Kept sets with a lower-case letter count everywhere but cannot be stored
 * (the encoder rejects them): their code is above 20^8. */
typedef struct kgx_sig kgx_sig;
typedef struct kgx_sig_record {
    uint64_t raw_key; /* the 8 bytes, first residue in the top byte */
    uint64_t code;    /* base-20 code; > 20^8 when not storable */
    int32_t function_index;
    uint32_t n_tuples; /* NSi: the set's size */
    uint32_t n_best;   /* NSiFj: its tuples of function_index */
    int32_t median_offset;
    float function_wt;
} kgx_sig_record;
typedef struct kgx_sig_stats {
    uint64_t n_windows; /* window positions of the labelled sequences, sum of max(0, len - 7) */
    uint64_t n_tuples;  /* those made of the 40 letters */
    uint64_t n_sets;
    uint64_t n_kept;     /* KS */
    uint64_t n_storable; /* kept and upper case */
    uint64_t n_seqs_with_signature; /* NSF */
    uint64_t num_sigs_rule; /* the builder's table size: its first listed prime above 3 * n_kept (0: none) */
} kgx_sig_stats;
/* residues / seq_offsets as in kgx_process_batch; seq_function[i] is the
 * function of sequence i, or negative for none (the sequence contributes
 * nothing); a value >= n_functions is KGX_ERANGE, as is a sequence longer
 * than 2^31-1.  The residues (1 byte per window) and the kept records (40
 * bytes each) are held in HBM; the tuples go through it in passes over
 * ascending, disjoint ranges of raw_key, each of at most max_pass_tuples
 * tuples (about 62 bytes per tuple of the largest pass).  max_pass_tuples 0 =
 * the smaller of 2^31-1 and what the device's free memory holds; above 2^31-1
 * it is KGX_EINVAL.  A corpus of at most max_pass_tuples windows is one pass.
 * A set is never split: one k-mer with more tuples than max_pass_tuples is
 * KGX_ERANGE (kgx_last_error names it).  The records, weights included, do
 * not depend on the passes.  KGX_ENOMEM when the residues, the largest pass
 * or the records do not fit.  KGX_EDEVICE without a gfx950 device: there is
 * no CPU path. */
int kgx_sig_select_passes(int device, const char *residues, const uint64_t *seq_offsets, const int32_t *seq_function,
                          uint32_t n_seq, uint32_t n_functions, uint64_t max_pass_tuples, kgx_sig **out);
/* kgx_sig_select_passes with max_pass_tuples 0 */
int kgx_sig_select(int device, const char *residues, const uint64_t *seq_offsets, const int32_t *seq_function,
                   uint32_t n_seq, uint32_t n_functions, kgx_sig **out);
/* the passes of the selection that held a tuple, in key order.  A pass that
 * was planned covers lo_key <= raw_key < hi_key; the single pass of a corpus
 * within the budget is not planned and reports lo_key 0, hi_key 2^64-1. */
typedef struct kgx_sig_pass {
    uint64_t lo_key, hi_key;
    uint64_t n_tuples, n_sets, n_kept;
} kgx_sig_pass;
int kgx_sig_pass_count(const kgx_sig *s, uint32_t *n);
int kgx_sig_pass_get(const kgx_sig *s, uint32_t i, kgx_sig_pass *out);
int kgx_sig_stats_get(const kgx_sig *s, kgx_sig_stats *out);
/* host view of the kept records in ascending raw_key order, valid until
 * kgx_sig_destroy */
int kgx_sig_records(kgx_sig *s, const kgx_sig_record **recs, uint64_t *n);
/* The image of the storable records (otu_index -1, avg_from_end =
 * (uint16_t)median_offset), inserted on the device as kgx_image_build
 * inserts; num_sigs 0 = the builder's rule.  KGX_EFULL as kgx_image_build. */
int kgx_sig_image(kgx_sig *s, uint64_t num_sigs, kgx_image **out, uint64_t *n_stored);
/* device time of the last selection's stages, in ms, summed over its passes:
 * upload, emit (with the planner's count launches), order (the two sorts),
 * segment (set heads, vote, keep test, bitmap), records (popcount,
 * compaction, weights) */
#define KGX_SIG_STAGES 5
int kgx_sig_stage_ms(const kgx_sig *s, float *ms);
int kgx_sig_destroy(kgx_sig *s);

/* ---- recall: labelled proteins back through an image ---- */
/* build_signature_kmers.cc's --recall-output / --validation-folder pass on
 * the device: every sequence runs through the context's image with
 * KGX_WANT_BEST, its best call is compared with its label, and the tallies
 * are made in HBM; hits and calls never reach the host.  seq_label[i] is an
 * index into the function index (>= 0), KGX_LABEL_OTHER (the id has a
 * function that is not in the index) or KGX_LABEL_NONE (the id has none).
 * Call classes, from kgx_best_call.kind: match (kind 1, fi0 == label),
 * mismatch (kind 1 otherwise), ambiguous (kind 2), none (kinds 0 and 3);
 * label classes: kept (>= 0), other, none. */
#define KGX_LABEL_OTHER (-1)
#define KGX_LABEL_NONE (-2)
#define KGX_RECALL_STAGES 4
typedef struct kgx_recall kgx_recall;
typedef struct kgx_recall_stats {
    uint64_t n_seq;
    uint64_t cell[3][4]; /* [label class][call class] in the orders above */
    uint64_t n_changed;
    uint64_t n_confusions;
    uint32_t n_pieces;
    float stage_ms[KGX_RECALL_STAGES]; /* upload, pass, tally, download; summed over the pieces */
} kgx_recall_stats;
typedef struct kgx_recall_function {
    uint32_t labelled; /* sequences labelled with the function */
    uint32_t correct;  /* of those, the matches */
    uint32_t called;   /* kind-1 calls of the function, whatever the label */
} kgx_recall_function;
typedef struct kgx_recall_pair {
    int32_t label, called;
    uint64_t count;
} kgx_recall_pair;
/* residues / seq_offsets as in kgx_process_batch (offsets need not start at
 * 0; a sequence is cut at its first NUL byte).  The corpus runs in pieces of
 * whole consecutive sequences: a piece is closed before the sequence that
 * would take its residues above piece_residues, so a longer sequence is a
 * piece of its own (0: 2^25 residues).  No result depends on the pieces.
 * Synchronous.  KGX_EINVAL for a null argument, offsets that decrease, or a
 * label below -2 or not below n_functions; KGX_ERANGE for more than 2^31-1
 * sequences, a piece above 2^40 residues, or a called function (fi0, fi1)
 * not below n_functions -- the image then belongs to another function index;
 * nothing is written out of bounds and no result is returned; KGX_EDEVICE
 * when the context's device is not gfx950.  n_seq 0 gives an empty result. */
int kgx_recall_run(kgx_ctx *ctx, const kgx_params *params, const char *residues, const uint64_t *seq_offsets,
                   const int32_t *seq_label, uint32_t n_seq, uint32_t n_functions, uint64_t piece_residues,
                   kgx_recall **out);
int kgx_recall_stats_get(const kgx_recall *r, kgx_recall_stats *out);
/* host views, valid until kgx_recall_destroy: the n_seq best calls in input
 * order; n_functions tallies; the changed sequences' indices, ascending (the
 * reference's "New" rows: call class none with a label other than
 * KGX_LABEL_NONE, kind 1 with fi0 != label, every kind 2); the distinct
 * (label, called) pairs of the kept / mismatch sequences, ascending by label,
 * then by called */
int kgx_recall_best(const kgx_recall *r, const kgx_best_call **best, uint64_t *n);
int kgx_recall_functions(const kgx_recall *r, const kgx_recall_function **fn, uint32_t *n);
int kgx_recall_changed(const kgx_recall *r, const uint32_t **seq, uint64_t *n);
int kgx_recall_confusions(const kgx_recall *r, const kgx_recall_pair **pairs, uint64_t *n);
int kgx_recall_destroy(kgx_recall *r);

/* ---- unique_prots: proteins grouped by their signature k-mer sets ---- */
/* unique_prots.cc on the device.  A sequence's set is the set of distinct
 * which_kmer values of its hits, taken before any scoring rule (no
 * kgx_params).  Sequences with equal sets form a group; members stand in
 * input order; groups are ordered as std::map orders std::set<u64> keys:
 * the ascending key lists compared lexicographically, a proper prefix before
 * the longer list, so the empty set's group, when there is one, is first.
 * Two sequences share a group iff their lists are equal key by key:
 * digest_bits (0..64) only sets how many bits of a list digest order the
 * grouping sort before lists are compared, and changes no result.
 * residues / seq_offsets / piece_residues as in kgx_recall_run; a piece is
 * also closed at 2^29 sequences.  Hits never reach the host.  Synchronous.
 * KGX_EINVAL for a null argument, offsets that decrease or digest_bits > 64;
 * KGX_ERANGE for more than 2^31-1 sequences or a piece of more than 2^31-1
 * residues; KGX_ENOMEM when the corpus's key lists do not fit the device;
 * KGX_EDEVICE when the context's device is not gfx950.  n_seq 0 gives an
 * empty result. */
#define KGX_UNIQ_STAGES 5 /* upload, pass (plan + probe), sets, group, download */
typedef struct kgx_uniq kgx_uniq;
typedef struct kgx_uniq_stats {
    uint64_t n_seq, n_hits, n_set_keys; /* hits before, keys after the per-sequence unique */
    uint64_t n_groups, n_empty, largest_group;
    uint64_t list_compares; /* comparator calls of the grouping sort that had to walk two lists (digest ties) */
    uint32_t n_pieces, digest_bits;
    float stage_ms[KGX_UNIQ_STAGES]; /* summed over the pieces */
} kgx_uniq_stats;
int kgx_uniq_run(kgx_ctx *ctx, const char *residues, const uint64_t *seq_offsets, uint32_t n_seq,
                 uint64_t piece_residues, uint32_t digest_bits, kgx_uniq **out);
int kgx_uniq_stats_get(const kgx_uniq *u, kgx_uniq_stats *out);
/* host views, valid until kgx_uniq_destroy: the groups as a CSR of sequence
 * indices (group_offsets[n_groups + 1]; indices ascend within a group); each
 * sequence's group; each group's ascending key list as a CSR in the same
 * group order (set_offsets[n_groups + 1]) */
int kgx_uniq_groups(const kgx_uniq *u, const uint64_t **group_offsets, const uint32_t **members, uint64_t *n_groups);
int kgx_uniq_group_of(const kgx_uniq *u, const uint32_t **group, uint64_t *n_seq);
int kgx_uniq_sets(const kgx_uniq *u, const uint64_t **set_offsets, const uint64_t **keys, uint64_t *n_groups);
int kgx_uniq_destroy(kgx_uniq *u);

/* ---- contexts: one per host thread, like one KmerGuts per pool thread --- */
/* The environment variable KGX_PROBE_DEFER, read when a context is created,
 * picks the form of its line probe over a line index with marks: 1 or unset,
 * every 64-window slice runs its first round and the tile's chains that left
 * their first line are then walked together, 16 to a load instruction; 0,
 * each slice runs all its rounds itself.  Same results either way (an A/B
 * switch); any other value is KGX_EINVAL and no context is made. */
int kgx_ctx_create(kgx_image *img, kgx_ctx **out);
int kgx_ctx_destroy(kgx_ctx *ctx);
/* the HIP stream the context launches on (hipStream_t) */
void *kgx_ctx_stream(kgx_ctx *ctx);
/* tuning knobs (results never change): "probe_variant" 0 = load key and
 * payload of every bucket examined, 1 = keys first (the 8-byte key, or the
 * packed record's low word), payload of the matching bucket only; -1 =
 * the fastest for the image (default: 2 for PACKED16, 0 for PACKED16 with a
 * presence filter, 1 for AOS24);
 * 2 / 3 = PACKED16 without a presence filter: groups of 4 / 8 lanes read one
 * aligned 64-B / 128-B table line per instruction (probe_j 1-4 / 1-2; other
 * combinations run variant 0);
 * "probe_filter" 1 (default) / 0 = use / ignore the image's presence filter;
 * "line_index" 1 (default) / 0 = this context's probes read the image's line
 * index when it has one / the reference slots (in-process A/Bs);
 * "probe_nt" 0 (default) / 1 = the line probe writes its hit records and mask
 * with non-temporal stores;
 * "plan_fused" 0 (default) = the plan (window bases, tile owners) in three
 * launches (reduce, scan, fill); 1 = one launch, a decoupled look-back over
 * workgroups (measured slower beside a probe: its waiting workgroups);
 * 2 = one workgroup of 1,024 threads (batches of up to 2^18 sequences);
 * "probe_serialize" 1 (default) / 0: this context's probes wait for the
 * image's previous probe (any context), so that probes run back to back and
 * the other kernels of the contexts overlap them;
 * "microbench_span" = bytes of the table kgx_microbench_random_read covers
 * (0 = all), "microbench_ilp" (1, 2, 4, 8, 16) reads in flight per lane and
 * "microbench_wgs" (1..32) 256-thread workgroups per CU;
 * "probe_j" = windows per lane (1, 2, 3, 4, 5 or 8, default 2; a tile
 * is 64 * probe_j windows), read at the next plan;
 * "fq_probe_j" (0..4, default 1) = windows per lane of kgx_fq_run_device's
 * DNA probe (fragments as anchors), 0 = probe_j;
 * "fq_fused" 1 (default) = the anchor fragment pass (fq_residues 0) counts,
 * scans and writes in one launch (decoupled look-back over tiles of 64
 * reads), 0 = count, scan, tail and anchor kernels;
 * "fq_plan" 1 (default) = kgx_fq_run_device plans the fragments of the
 * context's own fragment pass with one elementwise kernel (each has >= 11
 * residues, so a window base is its residue offset - 8 per earlier fragment),
 * 0 = the general plan (reduce, scan, scan);
 * "probe_stream" 1 = the image's chained probes all on one image-wide stream
 * (default 0: each on its context's stream, chained by events; same speed);
 * "probe_persist" (0..32, default 0) caps the line probe's grid at that many
 * workgroups per CU, its waves then striding over the tiles (measured slower,
 * DESIGN.md §5);
 * "score_variant" 0 (default) = hybrid run scorer: one lane per sequence,
 * except sequences of 2,049..39,998 windows, which the wave-parallel scorer
 * takes (a lane walking a 30k-aa protein would hold the stage for ms);
 * 1 = the wave-parallel scorer for every sequence (ballots over 64 queued
 * hits, serial f32 sums only); 2 = lanes only.  The wave scorer needs
 * order_constraint 0 (else lanes).  Results are identical;
 * "score_wave_tiles" (1..256, default 16) = probe tiles of windows per wave;
 * "score_lean" (0, 1 or 2, default 1): the lane scorer for calls without
 * KGX_WANT_OTU under order_constraint 0 (what lookup_request asks for) as a
 * kernel of its own that reads two dwords of each hit record and holds at
 * most 64 registers, so that it fits beside the probe wave for wave (1), and
 * with the lanes whose sequences pass min_hits packed into whole waves of
 * their workgroup (2: measured no faster than 1, profiles/TRIED.md); 0 = the
 * general kernel for every request.  Same results with each.  The
 * environment variable KGX_SCORE_LEAN (0, 1 or 2), read when a context is
 * created, sets its default for that context;
 * "fq_count" 1 (default) = the fq count pass scans stop codons one lane per
 * read, 0 = it translates like the emit pass (one wave per read);
 * "fq_residues" 1 (default) = kgx_fq_fragments writes the fragments'
 * residues; 0 = fragment anchors only (see kgx_fragments), for
 * kgx_fq_run_device;
 * "host_chunks" (1..64, default 6): kgx_process_batch splits a batch into up
 * to this many residue-balanced chunks of whole sequences (at least 2M
 * residues each; with "host_taper" 1, the default, the first and last are
 * half the others), alternating between the context and a twin context it
 * creates on first use, so that one chunk's D2H overlaps later chunks' H2D and
 * kernels; "host_copy" 1 (default) / 0: a chunk's results reach the host by
 * device stores into mapped pinned memory ("host_copy_blocks" workgroups,
 * default 64) / by DMA (hipMemcpyAsync).  PACKED16 images with hits wanted
 * ("host_hits16" 1, the default): hits cross PCIe as table records without
 * position or sequence (12 bytes with "host_rec12" 1, the default, the key
 * re-encoded on the host from the residues; else the 16-B records) plus the
 * batch's hit mask, and "host_threads" (default 12) host threads expand them
 * into kgx_hit records while later chunks stream ("host_nt" 1: with streaming
 * stores).  "host_h2d_first" 1 (default): a chunk's D2H starts once the next
 * chunk's residues are up (an H2D beside the D2H's stores is slowed 3-4x).
 * "host_stage_all" 1: every chunk is staged into pinned memory of its own, so
 * staging never waits for an earlier chunk's H2D (0, the default: the two
 * contexts' staging buffers, each reused once its last H2D is done; the same
 * batch time).
 * "pinned_input" 1 (default): a streamed batch whose residues already lie in
 * pinned, device-mapped host memory (kgx_host_alloc, hipHostMalloc,
 * hipHostRegister) is read by DMA straight from the caller's buffer -- no
 * staging copy on the host; a device scan looks for NUL bytes, and a batch
 * with one reruns staged, cut at the NUL as always (kgx_ctx_stat
 * "pinned_batches", "nul_reruns").
 * "host_stream_dma" 1: the streamed chunks' copies by DMA, each host region
 * copied whole at its room (0, the default: device stores of the counted
 * records into mapped memory).
 * "host_upload_stream" 1: chunks go up on a stream of their own into
 * per-batch device regions as soon as they are staged (0, the default: on
 * the context's stream, behind the chunk before).  "host_score_variant" (default 1,
 * the wave scorer; -1: the context's "score_variant"): the streamed chunks'
 * scorer.
 * "host_stream" 1 (default): chunks need no host round trip -- CSR offsets
 * are scanned on the device and the bulk copies (on a separate copy stream)
 * are sized on the device into host regions sized from the hit / call / OTU
 * rates of earlier batches; a batch that overflows them reruns on the exact
 * schedule (host_stream 0: counts to the host, then gather and copy, with
 * "counts_first" 1 holding chunk k's bulk copy until chunk k+1's counts are
 * out).  "stage_threads" (default 8): threads copying the caller's residues
 * into pinned staging.  "small_batch" (0..2^24 residues, default 2^21; 0 =
 * off): a one-chunk batch of at most this many residues is planned on the
 * host, read by the device from mapped pinned staging and its results stored
 * into mapped memory -- one host wait, no DMA copy (process_aa_seq's
 * latency), scored by the wave scorer unless "small_wave" is 0, with "small_wave_tiles"
 * (default 1) probe tiles per scorer wave.
 * "small_fused" 1 (default 0): such a batch runs as ONE launch when the image
 * is PACKED16, want is within HITS | CALLS, order_constraint is 0, min_hits
 * >= 1 and no sequence has more than 2,048 windows -- one workgroup per
 * sequence encodes, probes, scores and stores its records into mapped memory
 * (kgx_fused.hip); nothing of the batch stays on the device, so it is for
 * per-sequence callers (the facade's process_aa_seq), not for a batch that
 * kgx_kmap_add_hits / kgx_matrix_add_hits reads.  Results are
 * identical under every setting.  After a
 * chunked batch the device results are split over the two contexts:
 * kgx_kmap_add_hits / kgx_matrix_add_hits need a one-pass batch (host_chunks
 * 1, or want 0, which never chunks).
 * "gunzip_device" 1 / 0 (default): kgx_gunzip inflates blocked gzip members
 * on the device / on up to 16 host threads (the same decoder source).  The
 * device path is the faster one measured (17 against 5.8 GB/s of text, BGZF
 * level 6); the default is 0 because it did not clear the
 * bar set for it at level 1 (16 x one-thread zlib).  KGX_GUNZIP_DEVICE=0|1 in
 * the environment sets the default of new contexts.
 * "fq_parse_device" 0 (default) / 1: kgx_f2p_process frames a part's FASTQ
 * text with the host's strict parser / on the device (kgx_fq_parse); read when
 * a file starts; the output does not change.  KGX_FQ_PARSE_DEVICE=0|1 in the
 * environment sets the default of new contexts.
 * "fq_body_device" 0 (default) / 1: the fq handler (kgx_fq_process) frames a
 * request's FASTQ text on host threads / on the device (kgx_fq_parse, lenient),
 * part by part, the unconsumed text carried in front of the next part; a gzip
 * body's blocked members are then inflated on the device straight into the
 * text the parser reads (kgx_gunzip_device, whatever "gunzip_device" says),
 * and the ids of the reads it prints come down through kgx_fq_read_ids.  Read
 * from the handler's own context when a request starts; the output bytes do
 * not change.  KGX_FQ_BODY_DEVICE=0|1 in the environment sets
 * the default of new contexts */
int kgx_ctx_set_option(kgx_ctx *ctx, const char *name, int64_t value);
/* the option's current value; KGX_EINVAL for an unknown name */
int kgx_ctx_get_option(kgx_ctx *ctx, const char *name, int64_t *value);
/* counters of the context since its creation: "fused_batches" / "small_batches"
 * (small host batches that took the one-launch path / the one-wait path),
 * "stream_fallbacks" (streamed batches rerun exact after a region overflow or
 * a NUL in pinned input), "pinned_batches" (streamed batches read straight from
 * the caller's pinned residues), "nul_reruns", "lean_scores" (score stages
 * whose lane scorer was the lean kernel, option "score_lean"), "fq_parses"
 * (non-empty texts framed on the device, kgx_fq_parse / kgx_fq_parse_device) */
int kgx_ctx_stat(kgx_ctx *ctx, const char *name, int64_t *value);
/* launch on a caller-owned stream instead (hipStream_t; NULL = own stream) */
int kgx_ctx_set_stream(kgx_ctx *ctx, void *stream);

/* Host-buffer batch: process_aa_seq (kguts.cc:888-908) for every sequence of
 * the batch.  residues: concatenated sequence bytes; seq_offsets[n_seq+1]
 * delimits them.  Each sequence is cut at its first NUL byte, as
 * gather_hits' strlen() bound does (kguts.cc:792).  Synchronous; the result
 * views stay valid until the next call on ctx.  Large batches run in chunks
 * (option "host_chunks"); the results are the same. */
int kgx_process_batch(kgx_ctx *ctx, const kgx_params *params, const char *residues,
                      const uint64_t *seq_offsets, uint32_t n_seq, uint32_t want,
                      kgx_result *out);

/* ---- compact host results ----------------------------------------------
 * What crosses PCIe, handed over without building 32-byte kgx_hit records
 * (239 MB per 30M-residue C2 batch): per hit a record of the matched table
 * bucket without its key, plus one hit-mask bit per window.  A hit's window
 * -- hence its sequence and position -- is its mask bit, and its key is the
 * window's 8-mer, re-encoded from the caller's residues.  The hits come in
 * chunks of consecutive sequences:
 *   records        record_words (3 or 4) 32-bit words per hit, CSR order:
 *                  hit j of the batch (hit_offsets numbering) is at
 *                  records + record_words * (j - hit_begin); the words are
 *                  the PACKED16 bucket minus the key bits and
 *                  are opaque: kgx_compact_expand decodes them
 *   mask           chunk window w hit <=> bit w % 64 of mask[w / 64]
 *   window_start   sequence s's first chunk window is window_start[s -
 *                  seq_begin]; it owns max(0, len - 8) windows
 * hit_in_sequence_t (kguts.h:228-233) for any hit is thus built on the fly,
 * which is how the KmerGuts facade replays hit_cb (kguts.cc:814-815). */
typedef struct kgx_hit_chunk {
    uint32_t seq_begin, seq_end; /* the chunk's sequences [seq_begin, seq_end) */
    uint32_t record_words;
    uint32_t reserved;
    uint64_t hit_begin;
    const uint32_t *records;
    const uint64_t *mask;
    const uint64_t *window_start;
} kgx_hit_chunk;
typedef struct kgx_compact_result {
    /* offsets, calls, OTUs, best calls and n_windows as kgx_result; r.hits is
     * NULL when the hits are compact (n_chunks > 0), else (a batch that took
     * a path without compact records: small, one-pass or AOS24) the kgx_hit
     * records themselves, with n_chunks 0 */
    kgx_result r;
    uint32_t n_chunks;
    const kgx_hit_chunk *chunks;
} kgx_compact_result;
/* kgx_process_batch with compact hits: the same offsets, calls, OTUs and best
 * calls; the hits stay as the compact records (no kgx_hit expansion on the
 * host).  Views owned by ctx, valid until its next call. */
int kgx_process_batch_compact(kgx_ctx *ctx, const kgx_params *params, const char *residues,
                              const uint64_t *seq_offsets, uint32_t n_seq, uint32_t want,
                              kgx_compact_result *out);
/* kgx_hit records of sequences [s_begin, s_end) of a compact result into out
 * (out[0] = the first hit of s_begin; hit_offsets[s_end] - hit_offsets[s_begin]
 * records), kgx_hit.seq = batch index + seq_base.  residues / seq_offsets are
 * the batch's, as passed to the call that produced r.  Thread-safe (reads r
 * only): ranges may be expanded on several threads at once. */
int kgx_compact_expand(const kgx_compact_result *r, const char *residues, const uint64_t *seq_offsets,
                       uint32_t s_begin, uint32_t s_end, uint32_t seq_base, kgx_hit *out);

/* Resident call service: KmerGuts::process_aa_seq for ONE sequence
 * (kguts.cc:888-908) without a kernel launch per call -- for worker pools
 * that call per sequence (threadpool.cc:18-44, lookup_request.cc:153-172).
 * Persistent workgroups on the image's device, one per slot, poll slots in
 * mapped host memory; the call writes its sequence into a free slot and spins
 * until the device has stored its records.  Thread-safe; started on the first
 * call; instances of the workgroups last life_us each and the host keeps one
 * queued behind the running one while calls arrive, so the service leaves the
 * GPU within 2 x life_us of the last call (restarted on demand).  Serves
 * PACKED16 images, want within KGX_WANT_HITS | KGX_WANT_CALLS | KGX_WANT_OTU,
 * order_constraint 0, min_hits >= 1, sequences of at most 2,056 residues;
 * anything else, or every slot busy, returns KGX_EBUSY and the caller takes a
 * batch path (kgx_process_batch*).  Results as kgx_process_batch gives them
 * for a batch of this one sequence (kgx_hit.seq = 0, hits in position order;
 * OTU pairs in otus_by_count order); hits_cap / calls_cap / otus_cap must be
 * at least the sequence's window count (len - 8) for what want asks. */
int kgx_svc_call(kgx_image *img, const kgx_params *params, const char *seq, uint64_t len, uint32_t want,
                 kgx_hit *hits, uint64_t hits_cap, uint64_t *n_hits, kgx_call *calls, uint64_t calls_cap,
                 uint64_t *n_calls, kgx_otu *otus, uint64_t otus_cap, uint64_t *n_otus);
/* slots (1..64, default 32) and life_us (default 1000: an instance's stay
 * before the next one, already enqueued, takes over; bounds how long the
 * service holds its hardware queue); stops a running service (as
 * kgx_svc_stop) and applies the settings in one step, so the next call starts
 * the service with them.  idle_us is checked (>= 10, <= life_us) and ignored:
 * a per-workgroup idle exit could strand a quiet slot's next request
 * (DESIGN.md §8.8).  The KGX_SVC_LIFE_US environment default applies only to
 * images this was never called for. */
int kgx_svc_config(kgx_image *img, uint32_t slots, uint32_t idle_us, uint32_t life_us);
/* Stops the service: its workgroups leave and its memory is freed (so do
 * kgx_svc_config, kgx_image_set_layout / set_filter and kgx_image_close).
 * Safe while other threads are inside kgx_svc_call: it waits until they have
 * returned (their calls are served); a call that starts afterwards starts a
 * new service.  A call that gets no answer within 10 s (KGX_SVC_TIMEOUT_MS)
 * returns KGX_EDEVICE and leaves its slot for good (a late answer may still
 * land in it) and the service "broken": every later call, and every call
 * still waiting, returns KGX_EBUSY (take a batch path) until kgx_svc_stop or
 * kgx_svc_config replaces the service.  Stopping never waits on the runtime
 * without a bound: it waits at most 2 s for the workgroups to leave, and a
 * service whose workgroups did not is left allocated ("leaked") rather than
 * freed under them.  A request whose residues never reached the device
 * returns KGX_EBUSY. */
int kgx_svc_stop(kgx_image *img);
/* "slots", "calls" (served), "launches" (instances enqueued), "busy" (calls
 * turned away for want of a slot), "abandoned" (slots given up after a 10-s
 * wait), "broken" (1: calls are turned away until the service is replaced),
 * "leaked" (process-wide: stopped services whose workgroups did not leave
 * within 2 s, their memory kept),
 * "devmem" (1: requests are written into fine-grained device memory through a
 * large BAR, else mapped host memory; KGX_SVC_DEVMEM=0 forces the latter),
 * "priority" (100 + the service stream's priority; the stream is created at
 * the device's highest priority, so it has a hardware queue of its own and
 * batch streams never queue behind the persistent instances;
 * KGX_SVC_PRIORITY=normal gives it a normal stream),
 * "phase_n0".."phase_n15" (with KGX_SVC_DEBUG=1: summed ns of the host wall per
 * call, the device phases, the OTU tally of calls that want it and the
 * tally's final sort by count; n8 the probe rounds x 1000, n9 the probe's
 * first round, n10 its keys and homes, n11 thread 0's first-round loads,
 * n12 / n13 the scorer's first chunk's runs / sums, n14 the final system
 * fence: what is left of the results' stores to host memory, n15 the OTU
 * sort's shader clock cycles: n15 / n7 its clock) */
int kgx_svc_stat(kgx_image *img, const char *name, uint64_t *value);

/* Host-side profile of the context's last kgx_process_batch* call with option
 * "host_profile" 1 (HIP events per chunk; otherwise zeros).  Device stages are
 * sums over the batch's chunks of HIP-event intervals; host stages are wall
 * times on the host (expand_ms summed over the expansion threads). */
typedef struct kgx_host_profile {
    uint32_t chunks;
    uint32_t streamed;   /* 1: the streamed schedule (no host round trip per chunk) */
    double wall_ms;      /* the whole call */
    double stage_ms;     /* caller residues -> pinned staging (host copy) */
    double h2d_ms;       /* staged residues -> HBM */
    double device_ms;    /* plan + probe + score */
    double gather_ms;    /* count scan + gather into dense buffers */
    double d2h_ms;       /* the bulk copy to pinned host memory (from gather end, incl. queueing) */
    double expand_ms;    /* kgx_hit records built on host threads (0 in compact mode) */
    uint64_t h2d_bytes;
    uint64_t d2h_bytes;
} kgx_host_profile;
int kgx_ctx_host_profile(kgx_ctx *ctx, kgx_host_profile *out);

/* Device-buffer batch: same computation on residues / offsets already in HBM
 * (NUL-free sequences), enqueued on the context's stream without host
 * synchronisation.  The results stay in HBM (kgx_device_result).
 * Preconditions (checked on the device): d_seq_offsets[0..n_seq] are
 * monotone, absolute indices into d_residues, and d_seq_offsets[n_seq] -
 * d_seq_offsets[0] <= n_residues (the buffers are sized from n_residues).  A
 * batch that breaks them is processed as empty (no out-of-bounds access);
 * kgx_ctx_check and kgx_device_batch_collect then return KGX_EINVAL. */
int kgx_run_device(kgx_ctx *ctx, const kgx_params *params, const uint8_t *d_residues,
                   const uint64_t *d_seq_offsets, uint32_t n_seq, uint64_t n_residues,
                   uint32_t want, kgx_device_result *out);

/* The stages kgx_run_device enqueues, for per-kernel timing:
 *   kgx_stage_plan   window/chunk bookkeeping (2 small kernels)
 *   kgx_stage_probe  encode + probe: the HBM random-access kernel
 *   kgx_stage_score  hit-run scorer (calls, OTU flags; find_best_call with KGX_WANT_BEST) */
int kgx_stage_plan(kgx_ctx *ctx, const uint64_t *d_seq_offsets, uint32_t n_seq, uint64_t n_residues);
/* waits for the context's stream; KGX_EINVAL when its last plan found bad
 * offsets (see kgx_run_device), else KGX_OK */
int kgx_ctx_check(kgx_ctx *ctx);
int kgx_stage_probe(kgx_ctx *ctx, const uint8_t *d_residues, const uint64_t *d_seq_offsets);
int kgx_stage_score(kgx_ctx *ctx, const kgx_params *params, uint32_t want);
int kgx_device_result_get(kgx_ctx *ctx, kgx_device_result *out);

/* Synthetic query batch generated in HBM (synth.py make_queries). */
int kgx_synth_queries(kgx_ctx *ctx, uint64_t image_n_keys, uint32_t n_seq, uint32_t length,
                      uint32_t x_permille, uint64_t q0, uint8_t *d_residues,
                      uint64_t *d_seq_offsets);

/* ---- pools: one batch split across GPUs --------------------------------
 * north_star: query batches are split across the GPUs of one node with no
 * collective (sequences are independent, lookup_request.cc:153; KmerGuts
 * state is per sequence, kguts.h:263-266).  A pool holds n_ctx contexts,
 * context i on images[i % n_images] (typically one replica per GPU), each
 * driven by its own host thread -- the reference's thread pool of KmerGuts
 * over one image (threadpool.cc:18-44), spread over the node's GPUs. */
typedef struct kgx_pool kgx_pool;
int kgx_pool_create(kgx_image *const *images, uint32_t n_images, uint32_t n_ctx, kgx_pool **out);
int kgx_pool_destroy(kgx_pool *pool);
uint32_t kgx_pool_size(const kgx_pool *pool);
/* context i of the pool (owned by the pool; options may be set on it) */
kgx_ctx *kgx_pool_ctx(kgx_pool *pool, uint32_t i);
/* kgx_process_batch over the pool: the batch is cut into contiguous,
 * residue-balanced shards of whole sequences (kgx_shard_cuts), one per
 * running context -- the first two contexts of each device (environment
 * KGX_POOL_PER_DEVICE; a host batch on more contexts of one device only
 * queues behind the others' waits in the process's few hardware queues) --
 * all at once, on every GPU, and the results are concatenated in input order:
 * the same CSR, the same bytes (kgx_hit.seq included) as one context
 * processing the whole batch.  The views are owned by the pool and valid
 * until its next call. */
int kgx_pool_process_batch(kgx_pool *pool, const kgx_params *params, const char *residues,
                           const uint64_t *seq_offsets, uint32_t n_seq, uint32_t want, kgx_result *out);
/* The same with compact hits (kgx_process_batch_compact): every shard's
 * chunks, renumbered into the whole batch (seq_begin / seq_end / hit_begin),
 * pointing into the shard contexts' pinned buffers -- no host copy of any
 * hit.  When some shard's hits did not come back compact, every shard's hits
 * are expanded into one kgx_hit array instead (r.hits, n_chunks 0). */
int kgx_pool_process_batch_compact(kgx_pool *pool, const kgx_params *params, const char *residues,
                                   const uint64_t *seq_offsets, uint32_t n_seq, uint32_t want,
                                   kgx_compact_result *out);
/* kgx_pool_lookup's map for each running context: the first of the maps
 * whose device (kgx_kmap_device; -1 for a missing map) is the context's --
 * pick[i] indexes map_device; KGX_EINVAL when a context's device has none.
 * Host only (no device needed). */
int kgx_pool_map_select(const int32_t *ctx_device, uint32_t n_ctx, const int32_t *map_device, uint32_t n_maps,
                        int32_t *pick);
/* NUMA placement (the reference binds each worker's thread and memory to a
 * node, numa.cc:13-42): every pool context's host thread is bound at creation
 * to the CPUs of its device's NUMA node that the process may use (its affinity
 * mask), so that the pinned staging it grows and the copies into it stay on
 * the device's socket (pinned host memory is placed by first touch of the
 * allocating thread's node).  KGX_POOL_NUMA=0 leaves the threads unbound.
 * kgx_pool_numa_node: the node context i's thread is bound to, -1 when it is
 * not (unknown node, no usable CPU of it, or binding off). */
int kgx_pool_numa_node(const kgx_pool *pool, uint32_t i);
/* the NUMA node of a device: /sys/bus/pci/devices/<bus id>/numa_node of its
 * PCI function (-1: unknown or no NUMA information) */
int kgx_device_numa_node(int device);
/* the CPUs of NUMA node `node` that this process may run on (its affinity
 * mask and the node's cpulist, /sys/devices/system/node/node<N>/cpulist):
 * their count, and the first cap of them in cpus (may be NULL).  Needs no
 * device. */
int kgx_numa_node_cpus(int node, uint32_t *cpus, uint32_t cap);
/* free and total HBM of a device (hipMemGetInfo) */
int kgx_device_memory(int device, uint64_t *free_bytes, uint64_t *total_bytes);
/* cut points of n_shards contiguous residue-balanced shards: shard i is
 * sequences [cuts[i], cuts[i+1]), cuts[0] = 0, cuts[n_shards] = n_seq; cut i
 * is the first sequence starting at or after residue (total * i / n_shards)
 * (close_kmers_amd/shard.py balanced_shards).  Shards may be empty. */
int kgx_shard_cuts(const uint64_t *seq_offsets, uint32_t n_seq, uint32_t n_shards, uint32_t *cuts);

/* ---- host-side rules on results (run on the CPU, no device needed) ------ */
/* find_best_call (kguts.cc:1008-1199) over one sequence's calls.  names /
 * n_names is the function.index table (function_at_index, kguts.h:361-366).
 * *function receives the called function (NUL-terminated, truncated to
 * function_cap).  *score_offset_set is 0 when the reference leaves
 * score_offset untouched (no calls). */
int kgx_find_best_call(const kgx_call *calls, size_t n_calls, const char *const *names,
                       int n_names, int32_t *function_index, char *function, size_t function_cap,
                       float *score, float *weighted_score, float *score_offset,
                       int *score_offset_set);

/* a float as the reference's iostreams print it (operator<< at the default
 * precision: printf's %.6g of the value widened to double), NUL-terminated
 * into out (cap bytes); returns the full length.  Host only. */
size_t kgx_format_g6(float v, char *out, size_t cap);

/* find_best_call for many sequences at once, on the context's device:
 * sequence s owns calls[call_offsets[s] .. call_offsets[s+1]) (host arrays);
 * out[n_seq] receives each decision (kgx_best_call).  Synchronous. */
int kgx_find_best_calls(kgx_ctx *ctx, const kgx_call *calls, const uint64_t *call_offsets, uint32_t n_seq,
                        kgx_best_call *out);

/* Random-access ceiling of the context's image buffer: about n_reads
 * uniformly random records of the resident table read with many loads in
 * flight.  mode 0: a whole 24-byte bucket (key + payload, the AOS24 probe's
 * access), 1: the 8-byte key of a 24-byte bucket, 2: one aligned 64-byte
 * sector, 3: one aligned 16-byte record (the PACKED16 probe's access),
 * 4 / 5: one aligned 64-byte / 128-byte line read cooperatively by 4 / 8
 * lanes, 16 B each, in one instruction.  *ms = kernel time (HIP events),
 * *reads = records (modes 0-3) or lines (modes 4-5) actually read. */
int kgx_microbench_random_read(kgx_ctx *ctx, uint64_t n_reads, int mode, float *ms,
                               uint64_t *reads);

/* The current device batch's results (after kgx_run_device or the three
 * stages) as the host CSR kgx_process_batch returns; buffers as there. */
int kgx_device_batch_collect(kgx_ctx *ctx, uint32_t want, kgx_result *out);

/* ---- fq reads -> protein fragments (the fq handler's input side) --------
 * For every read and frame 1, 2, 3, -1, -2, -3 (DNASequence::
 * get_possible_proteins, dna_seq.cc:9-47): genetic code 11 translation
 * (trans_table.cc:36-84; codons with a base outside ACGTU/acgtu give 'X'),
 * split at '*', fragments longer than 10 residues kept
 * (fq_process_request.cc:329-343).  The fragments form a protein batch in
 * (read, frame, position) order, on the device, owned by ctx and valid until
 * the next fq call: feed it to kgx_fq_run_device (or, when residues is set,
 * kgx_run_device).
 *
 * With the context option "fq_residues" 0 (and a PACKED16 image probed by the
 * line probe, probe_j 1-4) the residues are not written: residues is NULL and
 * each fragment carries an anchor into the reads' bases instead, from which
 * kgx_fq_run_device's probe translates each window's 8 codons itself; read
 * and frame are NULL too (frame_counts gives both: read r's fragments are
 * frame_counts[6r..6r+5] of frames 1, 2, 3, -1, -2, -3 in turn). */
typedef struct kgx_fragments {
    uint32_t n_reads;
    uint32_t n_fragments;
    uint64_t n_residues;
    const uint8_t *residues;  /* device: fragment residues, concatenated (NULL: anchors) */
    const uint64_t *offsets;  /* device: [n_fragments + 1] */
    const uint32_t *read;     /* device: read index of each fragment (NULL with anchors) */
    const int8_t *frame;      /* device: frame of each fragment (NULL with anchors) */
    const uint32_t *frame_counts; /* device: fragments per (read, frame), [n_reads * 6] */
    const uint64_t *anchors;  /* device, when residues is NULL: per fragment (byte index in bases of its
                                 first codon's first base) << 1 | 1 on the reverse strand */
    const uint8_t *bases;     /* device: the reads' bases the anchors index */
    uint64_t n_bases;         /* bytes readable from bases */
} kgx_fragments;
/* reads from host memory (bases concatenated, read_offsets[n_reads + 1]) */
int kgx_fq_fragments(kgx_ctx *ctx, const char *bases, const uint64_t *read_offsets, uint32_t n_reads,
                     kgx_fragments *out);
/* kgx_fq_fragments in two steps, so that one block's upload overlaps earlier
 * blocks' work: _upload enqueues the H2D of the reads' bases and offsets on
 * ctx's stream and returns at once (bases in pinned memory go by DMA straight
 * from there and must stay unchanged until _uploaded returns; others are
 * staged first); _uploaded runs the fragment pass over them, as
 * kgx_fq_fragments does.  Nothing else may run on ctx between the two. */
int kgx_fq_upload(kgx_ctx *ctx, const char *bases, const uint64_t *read_offsets, uint32_t n_reads);
int kgx_fq_fragments_uploaded(kgx_ctx *ctx, kgx_fragments *out);
/* kgx_fq_fragments_uploaded in two halves: _start enqueues the fragment pass
 * over the uploaded reads behind their upload and returns at once;
 * kgx_fq_fragments_finish waits for it and fills out.  The fq handler starts
 * a part's pass as soon as its upload is enqueued, a part ahead of its
 * lookup, so the pass runs in the previous probe's tail and sizing the part
 * never holds the GPU idle between two probes.  The bases stay in use until
 * _finish returns; nothing else may run on ctx between the two calls. */
int kgx_fq_fragments_uploaded_start(kgx_ctx *ctx);
/* reads already in device memory */
int kgx_fq_fragments_device(kgx_ctx *ctx, const uint8_t *d_bases, const uint64_t *d_read_offsets,
                            uint32_t n_reads, kgx_fragments *out);
/* kgx_fq_fragments_device in two halves, for chunked streams of reads: _start
 * enqueues the fragment pass on ctx's stream and returns at once; _finish
 * waits for it and fills out (the same fragments).  Between the two the host
 * can enqueue other contexts' work -- the previous chunk's lookup -- so that
 * sizing one chunk never holds the GPU between two probes.  n_bases: the
 * caller's bound on the bytes the reads span and may read (d_read_offsets[0]
 * >= 0, d_read_offsets[n_reads] <= n_bases); a span past it is an error from
 * _finish, with nothing written past the buffers.  Nothing else may run on
 * ctx between the two calls. */
int kgx_fq_fragments_device_start(kgx_ctx *ctx, const uint8_t *d_bases, const uint64_t *d_read_offsets,
                                  uint32_t n_reads, uint64_t n_bases);
int kgx_fq_fragments_finish(kgx_ctx *ctx, kgx_fragments *out);
/* lookup + run scoring of a fragment batch: kgx_run_device over
 * (residues, offsets) when the residues were written, else plan, the probe
 * over the anchors (windows translated from the bases), score.  Same results. */
int kgx_fq_run_device(kgx_ctx *ctx, const kgx_params *params, const kgx_fragments *fragments, uint32_t want,
                      kgx_device_result *out);

/* After kgx_run_device over a kgx_fragments batch (with KGX_WANT_CALLS): only
 * the reads that have a call in some fragment, in read order, with what the
 * fq handler's frame choice reads of them (fq_process_request.cc:298-365):
 * per read its fragments per frame, per fragment its length and its calls.
 * Host views owned by the context, valid until its next call:
 *   reads[n]                       read indices
 *   frame_counts[6 n]              fragments per (read, frame)
 *   frag_offsets[n + 1]            read i's fragments [frag_offsets[i], frag_offsets[i+1])
 *   frag_len[...], call_offsets[...+1], calls[...]   per fragment */
typedef struct kgx_fq_called {
    uint32_t n;
    const uint32_t *reads;
    const uint32_t *frame_counts;
    const uint64_t *frag_offsets;
    const uint32_t *frag_len;
    const uint64_t *call_offsets;
    const kgx_call *calls;
} kgx_fq_called;
int kgx_fq_called_reads(kgx_ctx *ctx, const kgx_fragments *fragments, kgx_fq_called *out);

/* ---- the fq request handler (FqProcessRequest, fq_process_request.cc) ---
 * FASTQ text in, the handler's output lines out (per read: best frame,
 * score and the frame's family matches, fq_process_request.cc:298-365, over
 * FamilyMapper family_mapper.cc:46-205).  data_dir holds function.index and
 * otu.index; genus_file / families_file / nr_fasta (NULL or "" to skip) load
 * the family DB (KmerPegMapping::load_genus_map / load_families kmer.cc:
 * 341-493; NRLoader family mode nr_loader.cc:130-176, proteins in file
 * order).  Blocks are processed as the reference processes request blocks
 * (one FamilyMapper per block); `finished` marks the last block.  A request
 * whose first bytes are 1f 8b 08 is gzip (see below): each block's complete
 * members are inflated (kgx_gunzip) and their text processed as a block. */
typedef struct kgx_fq kgx_fq;
int kgx_fq_create(kgx_image *img, const char *data_dir, const char *genus_file, const char *families_file,
                  const char *nr_fasta, kgx_fq **out);
int kgx_fq_destroy(kgx_fq *fq);
/* *text: output lines of the block, owned by fq, valid until the next call */
int kgx_fq_process(kgx_fq *fq, const char *fastq, uint64_t n, int finished, const char **text,
                   uint64_t *text_len);
/* counters of the handler since its creation: "device_parts" / "host_parts"
 * (parts of text framed by kgx_fq_parse / parsed on the host: with option
 * "fq_body_device" 1 the host parses only what a request's last complete
 * record leaves, a record too long for the device, and a request handed over
 * as reads), "device_members" / "host_members" (gzip members inflated into the
 * parser's text on the device / to host text), "ids_fetched" (ids brought down
 * by kgx_fq_read_ids), "reads" (reads looked up), "tail_bytes_max" (the longest
 * text carried from one part to the next).  KGX_EINVAL for another name. */
int kgx_fq_stat(kgx_fq *fq, const char *name, uint64_t *value);

/* ---- reads -> six-frame protein FASTA (fastq_to_protein.cc)
 * For every read with a non-empty id, in input order, and each frame 1, 2, 3,
 * -1, -2, -3: the code-11 translation split at '*' as boost::split with
 * token_compress_on does (a run of '*' is one separator; a separator at either
 * end leaves an empty token there; an empty translation is one empty token),
 * the frame's tokens numbered 1, 2, ... and every token longer than 10 residues
 * written as
 *     >ID:FRAME:INDEX\nTOKEN\n
 * (fastq_to_protein.cc:24-47).  The fragments are kgx_fq_fragments' and come
 * in its (read, frame, position) order.  Reads and ids are host arrays (bases
 * and id bytes concatenated, read_offsets / id_offsets [n_reads + 1]); every
 * output is on the device, owned by ctx and valid until its next fq call. */
typedef struct kgx_fq_text {
    uint32_t n_reads;
    uint32_t n_fragments;
    uint64_t n_bytes;        /* length of text = offsets[n_fragments] */
    const char *text;        /* device: the records, back to back */
    const uint64_t *offsets; /* device: [n_fragments + 1] record starts in text */
    const uint32_t *read;    /* device: read index of each fragment */
    const int8_t *frame;     /* device: its frame */
    const uint32_t *token;   /* device: its INDEX, the token's number within the frame */
} kgx_fq_text;
int kgx_fq_proteins(kgx_ctx *ctx, const char *bases, const uint64_t *read_offsets, const char *ids,
                    const uint64_t *id_offsets, uint32_t n_reads, kgx_fq_text *out);

/* ---- FASTQ text -> reads, on the device (kgx_fq_parse.hip)
 * FastqParser::parse_char (fastq_parser.h:40-150) over text that begins at a
 * record boundary: the id runs to the first blank, a definition line may
 * follow it, the data line keeps its ASCII letters, the '+' line and the
 * quality line are skipped whatever they hold, and a record ends at its
 * quality line's newline.  An offending byte -- anything but '@' where a
 * record starts, a data byte that is neither a letter nor the newline ('\r'
 * and bytes >= 0x80 included), anything but '+' after the data line -- is
 * dropped and leaves the parser where it is.
 *
 * Without KGX_FQ_STRICT the reads are the records ended by their quality
 * newline, `consumed` is the end of the last of them (the caller feeds
 * text[consumed, n) again in front of what comes next) and the error is the
 * first offending byte before `consumed`, if any.  With KGX_FQ_STRICT the
 * first offending byte e ends the parse, as under fastq_to_protein's callback
 * (fastq_to_protein.cc:49-53): the reads are the records complete before e
 * and then the record in progress with the id and bases it has in [.., e), an
 * empty id included, and consumed = n.  With KGX_FQ_STRICT | KGX_FQ_FINISHED
 * and no error the record in progress is a read if and only if it has an id
 * (parse_complete) and consumed = n; with KGX_FQ_STRICT alone and no error
 * the result is the one without it.  The error's id is the last read's.  A
 * caller that parses a file in parts reports the line 1 + (the `newlines` of
 * the earlier calls) + error_newlines.
 *
 * bases, read_offsets, ids and id_offsets are the context's own buffers, the
 * ones kgx_fq_proteins fills (read_offsets[0] = id_offsets[0] = 0): they are
 * valid until the context's next fq call, and kgx_fq_proteins_device runs
 * kgx_fq_proteins' kernels over them without any copy.  bases and ids are
 * followed by 16 allocated bytes each, as kgx_fq_proteins leaves them; nothing
 * past bases[n_bases), ids[n_id_bytes) and the offsets' [n_reads + 1] is
 * defined (a record in progress that is no read leaves its bytes there).
 * d_text is device memory aligned to 16 bytes, of n bytes and no more; n is
 * at most KGX_FQ_PARSE_MAX (byte positions and the sums over them are 32-bit
 * on the device), KGX_ERANGE above it.  n = 0 gives zero reads and null
 * arrays; KGX_EINVAL for a null argument, an unaligned d_text or an unknown
 * flag.  Synchronous. */
#define KGX_FQ_STRICT 1u   /* the first offending byte ends the parse (fastq_to_protein.cc:49-53) */
#define KGX_FQ_FINISHED 2u /* the text ends the input (parse_complete) */
#define KGX_FQ_PARSE_MAX 0xFFFFF000ull
typedef struct kgx_fq_reads {
    uint32_t n_reads, n_reads_no_id;
    uint64_t n_bases, n_id_bytes;
    const uint8_t *bases;         /* device */
    const uint64_t *read_offsets; /* device: [n_reads + 1] */
    const uint8_t *ids;           /* device */
    const uint64_t *id_offsets;   /* device: [n_reads + 1] */
    uint64_t consumed;            /* the caller feeds text[consumed, n) again, in front of what comes next */
    uint64_t newlines;            /* '\n' in text[0, consumed) */
    uint32_t error;               /* 0 none, 1 starts with '>', 2 missing '@', 3 bad data character, 4 missing '+' */
    uint32_t error_byte;
    uint64_t error_pos, error_newlines; /* the first offending byte; '\n' in text[0, error_pos] */
    float upload_ms, parse_ms;          /* event times */
} kgx_fq_reads;
int kgx_fq_parse_device(kgx_ctx *ctx, const void *d_text, uint64_t n, uint32_t flags, kgx_fq_reads *out);
/* host text: uploaded (by DMA straight from pinned memory, kgx_host_alloc;
 * otherwise through the context's staging), then the above */
int kgx_fq_parse(kgx_ctx *ctx, const char *text, uint64_t n, uint32_t flags, kgx_fq_reads *out);
/* kgx_fq_proteins over the reads of this context's last kgx_fq_parse[_device]
 * call; KGX_EINVAL for reads that are not those */
int kgx_fq_proteins_device(kgx_ctx *ctx, const kgx_fq_reads *reads, kgx_fq_text *out);

/* ---- the ids of chosen reads of a device parse (kgx_fq_ids.hip, DESIGN.md
 * §8.14).  reads is this context's last kgx_fq_parse[_device] result (the
 * check kgx_fq_proteins_device makes, and that call's counts); read_index is
 * a host array of n read indices, strictly ascending, each below
 * reads->n_reads.  KGX_EINVAL otherwise, with nothing launched.  The chosen
 * reads' ids are gathered on the device (a length pass, its scan, a copy in
 * which 16 lanes move one id) and downloaded: ids[id_offsets[i],
 * id_offsets[i + 1]) is the id of read read_index[i].  n = 0 gives zero ids
 * (id_offsets[0] = 0) and launches nothing.  Synchronous. */
typedef struct kgx_fq_ids { /* host views owned by ctx, valid until its next fq call */
    uint32_t n;
    uint64_t n_bytes;
    const char *ids;            /* the chosen reads' id bytes, back to back */
    const uint64_t *id_offsets; /* [n + 1], id_offsets[0] = 0 */
} kgx_fq_ids;
int kgx_fq_read_ids(kgx_ctx *ctx, const kgx_fq_reads *reads, const uint32_t *read_index, uint32_t n,
                    kgx_fq_ids *out);

/* ---- FASTA text -> sequences, on the device (kgx_fa_parse.hip, DESIGN.md
 * §8.13).  FastaParser::parse_char (fasta_parser.h:38-144) over text that
 * begins at a record boundary: five states (start, id, defline, data,
 * id-or-data: the start of a line after the record's first data line).  '\r'
 * is skipped in every state and is no newline.  '>' opens a record from start
 * and from id-or-data; the id runs to the first blank (space or tab), a
 * definition line may follow it (not produced); in data a letter or '*' is a
 * residue, in id-or-data a letter is.  A record ends at the '>' that opens the
 * next one.  An offending byte leaves the parser where it is and is dropped:
 * 1 "Missing >": in start anything but '>', '\n' included; 2 "Bad data
 * character 'X'": in data anything but '\n', a letter or '*', so a '>' on the
 * line after a header is one and that second header's letters are residues of
 * the first record; 3 "Bad id or data character 'X'": in id-or-data anything
 * but '>', '\n' or a letter, so '*' first on a later line is one.  Bytes >=
 * 0x80 are neither letters nor blanks.
 *
 * Without flags the sequences are the records ended by a following '>',
 * `consumed` is the position of the last such '>' (0 when there is none: the
 * caller feeds text[consumed, n) again in front of what comes next, and a
 * re-fed tail starts with its '>', which puts the parser where it was),
 * `newlines` counts '\n' in text[0, consumed) and the error is the first
 * offending byte before `consumed`, if any; later ones are dropped, as the
 * reference's parser prints them and goes on.  With KGX_FA_FINISHED the
 * record in progress at the end of the text is a sequence too, whatever it
 * holds (parse_complete): n_seqs is the ends + 1, consumed = n, newlines
 * counts the whole text; an empty text is one record with an empty id and no
 * residues.  With KGX_FA_STRICT the first offending byte e ends the parse, as
 * under validate_fasta's callback (validate_fasta.cc:35-40): the sequences are
 * those of KGX_FA_FINISHED over text[0, e) -- the records complete before e,
 * then the record in progress as it stands, an empty id included --
 * consumed = n, newlines counts the whole text and error_newlines counts '\n'
 * in text[0, e].  KGX_FA_STRICT without an offending byte changes nothing.
 * The error's id is the last sequence's under KGX_FA_STRICT.  A caller that
 * parses a file in parts reports the line 1 + (the `newlines` of the earlier
 * calls) + error_newlines.
 *
 * residues, seq_offsets, ids and id_offsets are buffers of the context kept
 * for this call alone (seq_offsets[0] = id_offsets[0] = 0): they are valid
 * until the context's next kgx_fa_parse* call, across fq calls and across
 * kgx_run_device(ctx, params, residues, seq_offsets, n_seqs, n_residues, ..)
 * on the same context in particular.  residues and ids are followed by 16
 * allocated bytes each; nothing past residues[n_residues), ids[n_id_bytes)
 * and the offsets' [n_seqs + 1] is defined.  d_text is device memory aligned
 * to 16 bytes, of n bytes and no more; n is at most KGX_FA_PARSE_MAX (byte
 * positions and the sums over them are 32-bit on the device), KGX_ERANGE above
 * it, checked before anything is allocated.  n = 0 gives zero sequences and
 * null arrays without KGX_FA_FINISHED, and with it one empty record, both
 * offset arrays {0, 0}.  KGX_EINVAL for a null argument, an unaligned d_text
 * or an unknown flag; KGX_EDEVICE when the device's sums exceed what the text
 * allows.  Synchronous. */
#define KGX_FA_STRICT 1u   /* the first offending byte ends the parse (validate_fasta.cc:35-40) */
#define KGX_FA_FINISHED 2u /* the text ends the input (parse_complete) */
#define KGX_FA_PARSE_MAX 0xFFFFF000ull
typedef struct kgx_fa_seqs {
    uint32_t n_seqs, n_seqs_no_id;
    uint64_t n_residues, n_id_bytes;
    const uint8_t *residues;     /* device: what kgx_run_device takes */
    const uint64_t *seq_offsets; /* device: [n_seqs + 1] */
    const uint8_t *ids;          /* device */
    const uint64_t *id_offsets;  /* device: [n_seqs + 1] */
    uint64_t consumed;           /* the caller feeds text[consumed, n) again, in front of what comes next */
    uint64_t newlines;           /* '\n' in text[0, consumed) */
    uint32_t error;              /* 0 none, 1 missing '>', 2 bad data character, 3 bad id or data character */
    uint32_t error_byte;
    uint64_t error_pos, error_newlines; /* the first offending byte; '\n' in text[0, error_pos] */
    float upload_ms, parse_ms;          /* event times */
} kgx_fa_seqs;
int kgx_fa_parse_device(kgx_ctx *ctx, const void *d_text, uint64_t n, uint32_t flags, kgx_fa_seqs *out);
/* host text: uploaded (by DMA straight from pinned memory, kgx_host_alloc;
 * otherwise through the context's staging), then the above */
int kgx_fa_parse(kgx_ctx *ctx, const char *text, uint64_t n, uint32_t flags, kgx_fa_seqs *out);

/* The tool as a streaming handle: FASTQ text in, FASTA text out.  Blocks may
 * cut a record anywhere; `finished` ends the file and resets the parser and
 * the error state for the next one.  Records are framed as the fq handler
 * frames them, with the tool's two differences (fastq_parser.cc:17-36,
 * fastq_to_protein.cc:49-53): the first parse error ends the parse -- the
 * record in progress is translated with the id and bases it has and later
 * blocks of the file yield nothing -- and at the end of the input the record
 * in progress is translated if it has an id.  A file that starts 1f 8b 08 is
 * gzip, sniffed as kgx_fq_process sniffs it: each block's complete members are
 * inflated (kgx_gunzip on ctx) and their text processed.  part_bytes bounds
 * the FASTQ text taken per device pass (0: 32 MB, as the fq handler).  *text
 * is pinned host memory owned by the handle, valid until its next call.  One
 * context, no overlap of one part's download with the next part's kernels.
 *
 * With the context's option "fq_parse_device" at 1 (read when a file starts) a
 * part's text is uploaded and framed by kgx_fq_parse (KGX_FQ_STRICT, and
 * KGX_FQ_FINISHED on the file's last part) and translated by
 * kgx_fq_proteins_device; the host carries the part's unconsumed tail in
 * front of the next bytes, and a part that holds no complete record while
 * more input is to come is doubled instead of run again.  The text and every
 * stat but the clocks are the host parser's; `parts` counts the device passes
 * that held a read: more than the host path's where a part is part_bytes of
 * carried tail plus new text, fewer where parts had to grow to hold a record. */
typedef struct kgx_f2p kgx_f2p;
typedef struct kgx_f2p_stats { /* since create or the last file's `finished` call, that call included */
    uint64_t reads;            /* records parsed */
    uint64_t reads_no_id;      /* of them skipped for an empty id */
    uint64_t fragments;
    uint64_t text_bytes;
    uint64_t parts;            /* device passes */
    uint32_t error_line;       /* line of the parse error (0: none) */
    uint32_t gzip;             /* 1: the file was gzip */
    /* parse on the host (wall clock; "fq_parse_device" 1: the parse kernels'
     * event time, and upload_ms includes the text's upload); the others stream
     * time (HIP events) */
    double parse_ms, upload_ms, index_ms, sizes_ms, write_ms, download_ms;
} kgx_f2p_stats;
int kgx_f2p_create(kgx_ctx *ctx, uint64_t part_bytes, kgx_f2p **out);
int kgx_f2p_destroy(kgx_f2p *h);
int kgx_f2p_process(kgx_f2p *h, const char *fastq, uint64_t n, int finished, const char **text, uint64_t *text_len);
/* the file being read, or after `finished` the file just ended */
int kgx_f2p_get_stats(const kgx_f2p *h, kgx_f2p_stats *out);
/* the reference's report of that file's parse error, "Error found: ... at line
 * N id='...'" ("" if none); owned by the handle */
const char *kgx_f2p_error(const kgx_f2p *h);

/* ---- gzip (RFC 1952) and DEFLATE (RFC 1951) -------------------------------
 * The fq handler takes gzip bodies as the reference does
 * (fq_process_request.cc:64-104: a request whose first bytes are 1f 8b is
 * inflated before the FASTQ parser).  The decoder is the project's own
 * (csrc/kgx_inflate.h), one source for host and device; no zlib is linked.
 *
 * A member is *blocked* (BGZF, what bgzip/htslib write) when its extra field
 * holds a subfield "BC" of length 2: BSIZE = the member's total size - 1.  Its
 * extent is known without decoding, its ISIZE is at most 65,536, and such
 * members are inflated in parallel: one wave per member on the device
 * (inflate_members_kernel, option "gunzip_device" 1), or one host thread per
 * member ("gunzip_device" 0, the default).  A plain member's end is known only by decoding it; it is
 * decoded on the host, serially.  CRC-32 and ISIZE are verified for every
 * member.
 *
 * Behaviour where the reference is undefined: the reference's decoder stops at
 * the first member's end (zlib_support.cc:85-96), so a multi-member body
 * answers for its first member only and the rest is dropped silently.  Here
 * every member is decoded and the texts are concatenated (RFC 1952 2.2, and
 * what every gzip tool does); a single-member body gives the reference's
 * bytes exactly.  After at least one member, bytes that do not begin with
 * 1f 8b are ignored, as gzip ignores trailing garbage.
 *
 * Failure reasons (kgx_gz_status.reason, named in kgx_last_error()):
 * 1 block type 3, 2 stored LEN != ~NLEN, 3 over-subscribed code lengths,
 * 4 incomplete code lengths, 5 repeat with no previous length, 6 repeat past
 * HLIT + HDIST, 7 no end-of-block code, 8 length / distance symbol above
 * 285 / 29, 9 HLIT / HDIST too large, 10 invalid code, 11 distance before the
 * member's start, 12 input ends inside the stream, 13 output longer than
 * ISIZE (or than the room given), 14 output shorter than ISIZE, 15 CRC-32
 * mismatch; framing: 32 not gzip, 33 method not deflate, 34 reserved flag
 * bits, 35 member cut short, 36 BSIZE does not cover header and trailer,
 * 37 blocked member with ISIZE above 65,536, 38 header CRC.
 * Within the last 15 bits of a member's deflate data, 12 can stand for 10:
 * bits that are no code of an incomplete set, with fewer bits left than the
 * longest code has, are reported as the end of the input.  Host and device
 * report the same, and the member is refused either way. */
typedef struct kgx_inflate_stats {
    uint32_t stored_blocks, fixed_blocks, dynamic_blocks; /* blocks by type */
    uint32_t max_code_len; /* longest code length of a dynamic block's codes */
    uint32_t max_distance; /* largest match distance used */
    uint32_t max_length;   /* longest match */
    uint32_t overlap;      /* 1: some match overlapped its own output (distance < length) */
    uint32_t matches;
} kgx_inflate_stats;
typedef struct kgx_gz_member { /* one blocked member for the kernel */
    uint64_t in_off;  /* its deflate data (after the header) in the compressed bytes */
    uint64_t out_off; /* its slot in the output: the exclusive scan of the ISIZEs */
    uint32_t in_len;  /* deflate bytes (up to the trailer) */
    uint32_t out_len; /* ISIZE */
    uint32_t crc;     /* CRC-32 from the trailer */
    uint32_t reserved;
} kgx_gz_member;
typedef struct kgx_gz_status {
    uint32_t reason;  /* 0 = the member's bytes are in its slot and its CRC matched */
    uint32_t out_len; /* bytes produced */
    uint64_t bit_pos; /* input bit position (within the member's deflate data) of a failure */
} kgx_gz_status;
typedef struct kgx_gunzip_stats {
    kgx_inflate_stats inflate; /* over all members: counts summed, the others the maximum */
    uint64_t members, device_members, host_blocked_members, plain_members;
    uint64_t bytes_in, bytes_out;
    float upload_ms, kernel_ms, download_ms; /* event times of the device path */
    uint32_t reserved;
} kgx_gunzip_stats;
/* One raw deflate stream gz[0, n) into out[0, cap) on the calling thread; no
 * device needed.  KGX_OK, or KGX_EFORMAT with *reason and *bit_pos (out_len =
 * the bytes before the failure).  in_used = bytes of gz the stream took. */
int kgx_inflate_host(const void *gz, uint64_t n, void *out, uint64_t cap, uint64_t *out_len, uint64_t *in_used,
                     kgx_inflate_stats *stats, uint32_t *reason, uint64_t *bit_pos);
/* Framing only, no device: the complete blocked members at the front of
 * gz[0, n).  blocked = their number, out_bytes = the sum of their ISIZEs,
 * consumed = their bytes; members = blocked, plus 1 when the walk stopped at
 * a plain member's header.  A blocked member that is not complete yet stays
 * unconsumed; with `finished` it is KGX_EFORMAT.  Trailing bytes after at
 * least one member that do not begin with 1f 8b are consumed and ignored. */
int kgx_gunzip_scan(const void *gz, uint64_t n, int finished, uint64_t *members, uint64_t *blocked,
                    uint64_t *out_bytes, uint64_t *consumed);
/* gz[0, n) -> out[0, cap), host buffers.  Every complete member is decoded,
 * in order, the texts concatenated; consumed never splits a member.  Blocked
 * members go up to the device, through the kernel and back on ctx's stream
 * (option "gunzip_device" 1; 0, the default, and ctx NULL: up to 16 host threads); plain members are
 * decoded on the host, and only with `finished`: without it the walk stops in
 * front of a plain member (its end is not known), which costs the caller its
 * compressed size in memory until the last block.  cap too small: KGX_ERANGE,
 * nothing written past cap.  Bad data: KGX_EFORMAT, kgx_last_error() naming
 * the member index, the reason and the bit position.  stats may be NULL. */
int kgx_gunzip(kgx_ctx *ctx, const void *gz, uint64_t n, int finished, void *out, uint64_t cap, uint64_t *out_len,
               uint64_t *consumed, kgx_gunzip_stats *stats);
/* The kernel alone over device buffers: members[] (host) describes n_members
 * blocked members of d_gz; member m's bytes go to d_out + out_off.  status[]
 * (host, n_members) gets every member's outcome, member_stats[] (host, may be
 * NULL) its statistics, *kernel_ms (may be NULL) the kernel's event time.
 * d_gz must hold every [in_off, in_off + in_len) and d_out every [out_off,
 * out_off + out_len): the kernel touches nothing else.  KGX_OK, or KGX_EFORMAT
 * when some member failed (the others' outputs are intact). */
int kgx_gunzip_device(kgx_ctx *ctx, const void *d_gz, const kgx_gz_member *members, uint32_t n_members, void *d_out,
                      kgx_gz_status *status, kgx_inflate_stats *member_stats, float *kernel_ms);

/* ---- k-mer -> id tables in HBM ------------------------------------------
 * KmerPegMapping's kmer_to_id_ (kmer.h:84-127, filled by /add through
 * add_mapping, kmer.cc:173-210: every (k-mer, id) appended, duplicates kept)
 * and kmer_to_family_id_ (add_fam_mapping, kmer.cc:212-256: an id is added to
 * a k-mer's list once, lists in first-insertion order).  Ids are the
 * mapping's encoded ids (KmerPegMapping::encode_id); the id <-> name
 * dictionaries stay with the caller. */
typedef struct kgx_kmap kgx_kmap;
enum { KGX_KMAP_APPEND = 0, KGX_KMAP_SET = 1 };
int kgx_kmap_create(int device, int mode, kgx_kmap **out);
int kgx_kmap_destroy(kgx_kmap *map);
/* add (kmers[i], ids[i]) in order i = 0..n-1 (host arrays) */
int kgx_kmap_add(kgx_kmap *map, const uint64_t *kmers, const uint32_t *ids, uint64_t n);
/* add the hits of the context's last batch (want must have included HITS):
 * for each sequence s in order, each of its hits in position order adds
 * (hit.which_kmer, seq_ids[s]) -- the /add mapping step, add_request.cc:
 * 164-170 / 196-206.  seq_ids: host array of the batch's n_seq ids. */
int kgx_kmap_add_hits(kgx_kmap *map, kgx_ctx *ctx, const uint32_t *seq_ids);
uint64_t kgx_kmap_num_kmers(const kgx_kmap *map);
uint64_t kgx_kmap_num_values(const kgx_kmap *map);
/* host query: offsets[n+1] (CSR over the n k-mers) and, when ids != NULL,
 * the ids (ids_cap >= offsets[n]); unmapped k-mers have empty lists */
int kgx_kmap_lookup(kgx_kmap *map, const uint64_t *kmers, uint64_t n, uint64_t *offsets,
                    uint32_t *ids, uint64_t ids_cap);

/* ---- /lookup per-sequence rollups (LookupRequest::on_hit, lookup_request.cc:
 * 446-482; FamilyMapper::on_hit, family_mapper.cc:287-312) on the device ----
 * For each sequence s of the context's last batch (its hits still on the
 * device: kgx_process_batch / kgx_run_device / kgx_fq_run_device; any want),
 * each hit in position order, with L = map[hit.which_kmer] (no row: skipped):
 *   KGX_ROLLUP_FAMILY (kmer_to_family_id_): w = 1.0f / (float)|L|; for each
 *     id in L: row[id].hit_count++, .hit_total++, .weighted_total += w
 *   KGX_ROLLUP_PEG (kmer_to_id_): for each id in L: row[id].hit_count++
 * weighted_total is the f32 sum in that (hit) order.  A sequence's rows come
 * in the order its ids were first touched (hit order, then list order): a
 * caller that inserts them in that order into the request's one
 * std::unordered_map seq_score_ (cleared per sequence, as the reference does)
 * gets the map the reference's operator[] calls build, bucket by bucket, so
 * its iteration order too.  Buffers are owned by ctx and valid until its next
 * rollup. */
enum { KGX_ROLLUP_PEG = 0, KGX_ROLLUP_FAMILY = 1 };
typedef struct kgx_rollup_row { /* sequence_accumulated_score_t (lookup_request.h:26-42) + its key */
    uint32_t id;
    uint32_t hit_count;
    uint32_t hit_total;
    float weighted_total;
} kgx_rollup_row;
typedef struct kgx_rollup_result {
    uint32_t n_seq;
    const uint64_t *offsets;    /* [n_seq + 1]: sequence s's rows are [offsets[s], offsets[s+1]) */
    const kgx_rollup_row *rows; /* host */
    uint64_t n_events;          /* (hit, list entry) pairs folded */
} kgx_rollup_result;
int kgx_kmap_rollup(kgx_kmap *map, kgx_ctx *ctx, int mode, kgx_rollup_result *out);
/* the device the map lives on */
int kgx_kmap_device(const kgx_kmap *map);

/* /lookup's GPU side for a host batch on ONE context (a server worker's
 * request piece, lookup_request.cc:153-210,446-482): the pass and the rollup
 * over `map` (on the context's device) enqueued together -- upload, plan,
 * probe, score, the counts (and best calls) into mapped memory, the rollup
 * sized by the context's previous one -- and one host wait for both, instead
 * of kgx_process_batch's wait and then kgx_kmap_rollup's.  A batch
 * kgx_process_batch would run down its small-batch path (up to the context's
 * small_batch residues, 65,536 sequences, one chunk) runs down that path with
 * the rollup queued behind it; others take the one-pass path.  want within
 * KGX_WANT_CALLS | KGX_WANT_BEST; results as those two calls give them (out:
 * no hits; the views valid until the context's next call). */
int kgx_lookup(kgx_ctx *ctx, kgx_kmap *map, int mode, const kgx_params *params, const char *residues,
               const uint64_t *seq_offsets, uint32_t n_seq, uint32_t want, kgx_result *out,
               kgx_rollup_result *rollup);
/* /lookup's GPU side for a whole host batch over a pool
 * (LookupRequest::process_work + on_hit, lookup_request.cc:153-210,446-482):
 * the batch is cut into shards of whole sequences (up to twice as many per
 * device as kgx_pool_process_batch: a shard here is one pass, no twin; a
 * device's first and last shards half the others' residues), enqueued in
 * order on the pool's per-device pass, score and rollup streams with no host
 * wait; each runs on its context's buffers as ONE pass (its hits stay on the
 * device),
 * with want within KGX_WANT_CALLS | KGX_WANT_BEST (KGX_WANT_BEST: the
 * find_best_match decision), and then kgx_kmap_rollup over maps[j], the map on
 * that context's device (one map per device the pool spans).  Nothing per hit
 * crosses PCIe.  out: hit and call offsets, calls and best calls over the whole
 * batch (out->hits NULL); rollup: every sequence's rows in input order
 * (offsets over the batch), each sequence's rows in first-touch order as
 * kgx_kmap_rollup gives them.  Views owned by the pool, valid until its next
 * call. */
int kgx_pool_lookup(kgx_pool *pool, kgx_kmap *const *maps, uint32_t n_maps, int mode, const kgx_params *params,
                    const char *residues, const uint64_t *seq_offsets, uint32_t n_seq, uint32_t want,
                    kgx_result *out, kgx_rollup_result *rollup);

/* ---- /matrix pair counting (matrix_request.cc:83-190) --------------------
 * One kgx_matrix per /matrix request (the request's matrix_proteins_ and
 * distance_ state, matrix_request.h:25-26).  For each sequence s of a batch,
 * in order, with id e = seq_ids[s] (e joins the request's seen set first):
 * for every hit of s, for every id f in the hit k-mer's kmap list, if f != e
 * and f was seen in this request, distance_[(e, f)] += 1. */
typedef struct kgx_matrix kgx_matrix;
typedef struct kgx_pair_count { /* one distance_ entry */
    uint32_t id1, id2;
    uint64_t count;
} kgx_pair_count;
int kgx_matrix_create(kgx_kmap *map, kgx_matrix **out);
int kgx_matrix_destroy(kgx_matrix *mx);
/* add the context's last batch (want must have included HITS) */
int kgx_matrix_add_hits(kgx_matrix *mx, kgx_ctx *ctx, const uint32_t *seq_ids);
/* all pair counts so far, ordered by (id1, id2) as std::map iterates
 * distance_; the buffer is owned by mx and valid until the next call */
int kgx_matrix_pairs(kgx_matrix *mx, const kgx_pair_count **pairs, uint64_t *n_pairs);

/* ---- HIP-event timing on a context's stream ----------------------------- */
int kgx_event_create(void **event);
int kgx_event_destroy(void *event);
/* record on the stream `ctx` launches on */
int kgx_event_record(void *event, kgx_ctx *ctx);
/* milliseconds between two recorded events (waits for `end`) */
int kgx_event_elapsed_ms(void *start, void *end, float *ms);

/* Device memory helpers for callers without their own allocator. */
int kgx_device_alloc(int device, uint64_t nbytes, void **out);
int kgx_device_free(void *p);
/* Pinned (page-locked, portable) host memory.  Batch inputs that live in it
 * reach the device by DMA straight from there (kgx_fq_fragments skips its
 * staging copy for such bases). */
int kgx_host_alloc(uint64_t nbytes, void **out);
int kgx_host_free(void *p);
int kgx_memcpy_h2d(void *dst, const void *src, uint64_t nbytes);
int kgx_memcpy_d2h(void *dst, const void *src, uint64_t nbytes);
int kgx_ctx_synchronize(kgx_ctx *ctx);
/* n bytes from device memory to device memory, enqueued on ctx's stream:
 * ordered with ctx's other work, not waited for */
int kgx_ctx_memcpy_d2d(kgx_ctx *ctx, void *dst, const void *src, uint64_t nbytes);

#ifdef __cplusplus
}
#endif

#endif /* KGX_H */
