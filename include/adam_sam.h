/*
 * adam_sam.h -- SAM text into and out of the device around the BQSR path
 * (SURVEY.md §8 rows f1, f2, f3), part of libadam_bqsr.so.
 *
 *   ingest  : sc.adamLoad of a SAM file          adam-core/.../rdd/AdamContext.scala:122-137
 *             SAMRecordConverter.convert         adam-core/.../converters/SAMRecordConverter.scala:26-144
 *             RecordGroupDictionary (sorted ids) adam-core/.../models/RecordGroupDictionary.scala:36-43
 *             with the BQSR column projection    adam-core/.../projections/ADAMRecordField.scala:28-71
 *   output  : the recalibrated records written back (adamSave,
 *             adam-core/.../rdd/AdamRDDFunctions.scala:37-56) -- here as SAM
 *             text: every record's QUAL field replaced by the string
 *             RecalUtil.recalibrate built (trimmed length, Q13; Java chars
 *             as UTF-8, Q14), every other byte of the record kept
 *   dedup   : MarkDuplicates (adam-core/.../rdd/MarkDuplicates.scala:24-111),
 *             the `-mark_duplicate_reads` step `transform` runs before BQSR
 *             (adam-cli/.../cli/Transform.scala:73-76)
 *   flagstat: adamFlagStat (adam-core/.../rdd/FlagStat.scala:21-116), the
 *             counters `adam flagstat` prints, over a parse or Arrow buffers
 *   print_tags: adamCharacterizeTags / adamCharacterizeTagValues
 *             (adam-core/.../rdd/AdamRDDFunctions.scala:200-229), the tag and
 *             tag-value counts `adam print_tags` prints
 *   reads2ref: Reads2PileupProcessor (adam-core/.../rdd/Reads2PileupProcessor.scala:34-197),
 *             the ADAMPileup rows `adam reads2ref` writes
 *
 * Same conventions as adam_bqsr.h (bqsr_status results, bqsr_last_error(),
 * library-owned handles with *_destroy, `stream` = hipStream_t as void*).
 */
#ifndef ADAM_SAM_H
#define ADAM_SAM_H

#include "adam_bqsr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A parsed SAM file: the text and the record columns, in device memory. */
typedef struct bqsr_sam bqsr_sam;

/* Parse a whole SAM file (header + records) as read_sam does
 * (adam_amd/records.py, the SAMRecordConverter semantics): start = POS - 1
 * when RNAME is a header @SQ name and POS != 0; flag bits only when the flag
 * word is non-zero (quirk Q2); MD:Z -> mismatchingPositions; RG:Z -> the
 * index of the name among the sorted @RG IDs; referenceName ids in order of
 * first appearance.  Header lines are parsed on the host, records on the
 * device (line split, field split, CIGAR text -> BAM u32 elements).
 * `text` is host memory (pinned or not).  BQSR_ERR_SAM_PARSE where the
 * reference's parser throws (fewer than 11 fields, a tag without two ':', a
 * malformed CIGAR or FLAG / POS); BQSR_ERR_UNSUPPORTED for header lines after
 * the first record and lone '\r' bytes. */
bqsr_status bqsr_sam_parse(bqsr_context* ctx, const char* text, int64_t n_bytes, void* stream, bqsr_sam** out);
void bqsr_sam_destroy(bqsr_sam* s);
/* BAM bytes (BGZF) -> the same parse bqsr_sam_parse builds from the SAM
 * text of the same records (AdamContext.scala:122-137 adamBamLoad,
 * SAMRecordConverter.scala:26-144): BGZF blocks inflated (and their CRC32
 * checked) by host threads; on the device every record becomes its SAM text
 * line (integer tag types as "i", floats by Java's Float.toString, arrays as
 * B:t,...) and the lines go through the SAM record parser.  So every call
 * on a SAM parse -- rewrite, text download, MarkDuplicates, ADAM columns --
 * serves BAM input too. */
bqsr_status bqsr_bam_parse(bqsr_context* ctx, const uint8_t* bam, int64_t n_bytes, void* stream, bqsr_sam** out);
/* Which form of the BGZF inflate served a parse: 0 not a BAM parse, 1 the
 * host form (BQSR_TUNE_BGZF 0, or a file the device form declined), 2 the
 * device form. */
int32_t bqsr_sam_bam_form(const bqsr_sam* s);
/* The device form's inflate alone, with bqsr_bam_parse's code: the BGZF
 * members of `bgzf` (host memory) located, uploaded and inflated by the two
 * device passes; no BAM header or record work.  out (host, out_cap bytes)
 * receives the inflated stream, member i's bytes at the sum of the ISIZE
 * fields before it; block_status[i] (status_cap entries) is 0 for a member
 * that inflated to ISIZE bytes with its CRC32, non-zero for one the device
 * declines (its bytes in `out` are unspecified).  *out_len = the stream's
 * bytes, *n_blocks = the members; out == NULL returns only these two.
 * BQSR_ERR_SAM_PARSE for bytes that are no chain of BGZF members. */
bqsr_status bqsr_bgzf_inflate(bqsr_context* ctx, const uint8_t* bgzf, int64_t n_bytes, void* stream, uint8_t* out,
                              int64_t out_cap, int64_t* out_len, int32_t* block_status, int64_t status_cap,
                              int64_t* n_blocks);

typedef struct bqsr_sam_counts {
  int64_t n_reads;     /* records (empty lines skipped)   */
  int64_t seq_bytes;   /* Σ SEQ field lengths            */
  int64_t qual_bytes;  /* Σ QUAL field lengths           */
  int64_t cigar_ops;   /* Σ CIGAR elements               */
  int64_t md_bytes;    /* Σ MD:Z value lengths           */
  int64_t text_bytes;  /* the SAM text (input, or the rewritten text after bqsr_sam_rewrite_quals) */
  int32_t n_ref_names; /* distinct referenceNames used    */
  int32_t n_read_groups;
} bqsr_sam_counts;
bqsr_status bqsr_sam_get_counts(const bqsr_sam* s, bqsr_sam_counts* out);
/* referenceName i (ref_index order: first appearance in the records) */
const char* bqsr_sam_ref_name(const bqsr_sam* s, int32_t i);

/* The record columns (bqsr_records layout; ref_index as RecordBatch keeps it:
 * index into the bqsr_sam_ref_name list, -1 when referenceName is null). */
typedef struct bqsr_sam_columns {
  uint32_t* flags;
  int32_t* rg_id;
  int32_t* ref_index;
  int64_t* start;
  uint64_t* seq_offset;
  uint8_t* seq;
  uint64_t* qual_offset;
  uint8_t* qual;
  uint64_t* cigar_offset;
  uint32_t* cigar;
  uint64_t* md_offset;
  uint8_t* md;
} bqsr_sam_columns;
/* device pointers of the columns (valid while `s` lives) */
bqsr_status bqsr_sam_device_columns(const bqsr_sam* s, bqsr_sam_columns* out);
/* copy the columns to caller-allocated host arrays sized by bqsr_sam_get_counts */
bqsr_status bqsr_sam_download(const bqsr_sam* s, const bqsr_sam_columns* dst);

/* The parse's records as a BQSR batch, packed on the device: the layout,
 * launch window and read order bqsr_batch_create builds from the same
 * records' host columns (bqsr_sam_download), without the columns leaving the
 * device.  ref_contig[i] = the bqsr_sites contig index of referenceName i
 * (bqsr_sam_ref_name order) or BQSR_CONTIG_UNKNOWN; n_ref may be 0 (no known
 * sites).  The batch owns its columns (the parse may be destroyed).
 * BQSR_ERR_UNSUPPORTED as bqsr_batch_create (fields beyond 65535, a
 * recordGroupId beyond 65535, reads longer than the device path takes). */
bqsr_status bqsr_sam_batch_create(bqsr_context* ctx, const bqsr_sam* s, const int32_t* ref_contig, int32_t n_ref,
                                  void* stream, bqsr_batch** out);

/* ADAMRecord Parquet (§8 f1/f2): adamLoad with the BQSR projection
 * (core/rdd/AdamContext.scala:139-161, projections/Projection.scala:10-34) as
 * Arrow decodes it on the host -- the column buffers uploaded as they are and
 * turned into the parse layout on the device.  One bqsr_arrow_chunk per Arrow
 * record batch (array offsets 0); a NULL column is all null.  String columns:
 * int32 offsets [n+1], UTF-8 bytes, validity bitmap (NULL: all valid); chars
 * are Java chars (a 4-byte UTF-8 sequence is a surrogate pair): a qual char c
 * enters as the byte c & 0xFF, a sequence / MD char as min(c, 0xFF) (as
 * adam_amd/parquet.py).  CIGAR strings are parsed by samtools
 * TextCigarCodec's rules (BQSR_ERR_SAM_PARSE, read index, when malformed).
 * reference = referenceName dictionary indices (the caller's dictionary; the
 * ref_contig map of bqsr_arrow_batch_create is indexed by them).  Booleans: a
 * null reads as false. */
typedef struct bqsr_arrow_strings {
  const int32_t* offsets;
  const uint8_t* data;
  const uint8_t* validity;
} bqsr_arrow_strings;
typedef struct bqsr_arrow_chunk {
  int64_t n_reads;
  bqsr_arrow_strings sequence, qual, cigar, md; /* md = mismatchingPositions */
  const int32_t* reference;
  const uint8_t* reference_validity;
  const int64_t* start;
  const uint8_t* start_validity;
  const int32_t* record_group; /* recordGroupId */
  const uint8_t* record_group_validity;
  /* readPaired, readMapped, readNegativeStrand, secondOfPair, primaryAlignment, duplicateRead */
  const uint8_t* bools[6];
  const uint8_t* bools_validity[6];
  /* MarkDuplicates only (NULL otherwise): readName; referenceId (NULL: the
   * referenceName index); library = 1 + the rank of recordGroupLibrary among
   * the input's sorted distinct libraries, 0 for null */
  bqsr_arrow_strings read_name;
  const int32_t* reference_id;
  const uint8_t* reference_id_validity;
  const int32_t* library;
} bqsr_arrow_chunk;
typedef struct bqsr_arrow bqsr_arrow;
bqsr_status bqsr_arrow_load(bqsr_context* ctx, const bqsr_arrow_chunk* chunks, int32_t n_chunks, void* stream,
                            bqsr_arrow** out);
void bqsr_arrow_destroy(bqsr_arrow* a);
int64_t bqsr_arrow_reads(const bqsr_arrow* a);
/* the records as a BQSR batch (as bqsr_sam_batch_create) */
bqsr_status bqsr_arrow_batch_create(bqsr_context* ctx, const bqsr_arrow* a, const int32_t* ref_contig, int32_t n_ref,
                                    void* stream, bqsr_batch** out);
/* The qual column after apply (adamSave of the recalibrated records): per
 * read the recalibrated chars as UTF-8 (pass-through reads keep their input
 * string; null where the input had none and nothing was written), built on
 * the device; prepare returns the byte count, column copies the Arrow
 * buffers (int32 offsets [n+1], bytes, validity bitmap) to the host.  b ==
 * NULL keeps every input string. */
bqsr_status bqsr_arrow_qual_prepare(bqsr_context* ctx, bqsr_arrow* a, const bqsr_batch* b, const uint8_t* out_qual,
                                    const uint32_t* out_start, const uint32_t* out_len, const uint64_t* exceptions,
                                    int64_t n_exceptions, void* stream, int64_t* n_bytes);
bqsr_status bqsr_arrow_qual_column(const bqsr_arrow* a, int32_t* offsets, uint8_t* data, uint8_t* validity);
/* MarkDuplicates over the reads (bqsr_sam_mark_duplicates' rules; readName
 * and library from the chunk columns): the duplicateRead bits of the
 * records (and of the batches built after) set or cleared */
bqsr_status bqsr_arrow_mark_duplicates(bqsr_context* ctx, bqsr_arrow* a, int64_t* n_duplicates);
/* the reads' flag bit `flag` (a BQSR_F_* value) as an Arrow boolean bitmap */
bqsr_status bqsr_arrow_flag_bitmap(const bqsr_arrow* a, uint32_t flag, uint8_t* bitmap);

/* Output (§8 f2): replace every record's QUAL field by its recalibrated
 * string.  out_qual / out_start / out_len / exceptions are the device
 * buffers bqsr_apply_async wrote for batch `b`, built from this parse's
 * records in read order (b's slot of read r = its qual chars' base).
 * Recalibrated reads get the chars of [out_start, out_start + out_len) as
 * UTF-8 (chars above 0xFF from the exception list); pass-through reads keep
 * their QUAL bytes; with b == NULL every QUAL field is kept.  After
 * bqsr_sam_mark_duplicates the FLAG fields are rewritten too (0x400 = the
 * duplicateRead MarkDuplicates gave the read).  The header is kept, empty
 * lines are dropped and every record ends with '\n'.  The new text
 * replaces the parse's on the device. */
bqsr_status bqsr_sam_rewrite_quals(bqsr_context* ctx, bqsr_sam* s, const bqsr_batch* b, const uint8_t* out_qual,
                                   const uint32_t* out_start, const uint32_t* out_len, const uint64_t* exceptions,
                                   int64_t n_exceptions, void* stream);
/* copy the (rewritten) SAM text to host memory of at least counts.text_bytes */
bqsr_status bqsr_sam_text_download(const bqsr_sam* s, char* dst);

/* ADAMRecord columns (§8 f2: adamSave of SAMRecordConverter's records,
 * core/rdd/AdamRDDFunctions.scala:37-56, converters/SAMRecordConverter.scala:
 * 26-144) of records [r0, r0 + n) of the parse, from its current text (after
 * bqsr_sam_rewrite_quals: the recalibrated QUAL and MarkDuplicates' FLAG).
 * Record-level columns in Arrow layout, built on the device:
 *   strings (int32 offsets [n+1], bytes, validity bitmap): readName, sequence,
 *     cigar (re-encoded, "*" when empty), qual, mismatchingPositions (MD),
 *     attributes (every tag but MD as TG:T:value, descending binary tag,
 *     tab-joined; "" without tags);
 *   int32 (+ validity): referenceId, mapq, mateReferenceId, recordGroupId;
 *   int64 (+ validity): start, mateAlignmentStart;
 *   bitmaps: readPaired, properPair, readMapped, mateMapped,
 *     readNegativeStrand, mateNegativeStrand, firstOfPair, secondOfPair,
 *     primaryAlignment, failedVendorQualityChecks, duplicateRead.
 * Bitmaps are Arrow's (bit r of word r / 64, LSB first).  The columns that
 * depend only on the read group or the @SQ entry (referenceName,
 * recordGroup*, referenceLength / Url, mate*) come from the header text by
 * index (bqsr_sam_header_text).  An H or B tag, or an 'i' tag outside Int,
 * gives BQSR_ERR_UNSUPPORTED (the reference's attribute conversion throws).
 * prepare: pass 1 and the sizes; columns: pass 2 and the copies into the
 * caller's host buffers (NULL pointers skip a column). */
typedef struct bqsr_adam_sizes {
  int64_t n_reads;
  int64_t str_bytes[6];
  int64_t bitmap_words; /* u64 words of each bitmap */
} bqsr_adam_sizes;
typedef struct bqsr_adam_host {
  int32_t* str_offsets[6];
  uint8_t* str_bytes[6];
  uint64_t* str_valid[6];
  int32_t* i32[4];
  int64_t* i64[2];
  uint64_t* int_valid[6]; /* referenceId, mapq, mateReferenceId, recordGroupId, start, mateAlignmentStart */
  uint64_t* bools[11];
} bqsr_adam_host;
bqsr_status bqsr_sam_adam_prepare(bqsr_context* ctx, bqsr_sam* s, int64_t r0, int64_t n, void* stream,
                                  bqsr_adam_sizes* out);
bqsr_status bqsr_sam_adam_columns(bqsr_context* ctx, bqsr_sam* s, const bqsr_adam_host* dst, void* stream);
/* The same pass 2, the columns left on the device: *cols their DEVICE
 * addresses (nothing is copied), what bqsr_parquet_pages_size_strings / _bools
 * / _size encode from (transform -parquet_encoder device).  The addresses hold
 * until the next adam call on the parse. */
bqsr_status bqsr_sam_adam_device_columns(bqsr_context* ctx, bqsr_sam* s, bqsr_adam_host* cols, void* stream);
/* The ADAM columns' qual from an apply's outputs for batch `b` (built from
 * this parse in read order) instead of the text's QUAL, as
 * bqsr_sam_rewrite_quals would write them (pass-through reads keep theirs),
 * without rewriting the text; the device buffers must outlive the following
 * prepare / columns calls.  b == NULL: the text's QUAL again.  After
 * MarkDuplicates the duplicateRead column follows its bits either way. */
bqsr_status bqsr_sam_adam_set_quals(bqsr_context* ctx, bqsr_sam* s, const bqsr_batch* b, const uint8_t* out_qual,
                                    const uint32_t* out_start, const uint32_t* out_len, const uint64_t* exceptions,
                                    int64_t n_exceptions, void* stream);
/* the header lines of the parse (SAM input, or a BAM's header text) */
bqsr_status bqsr_sam_header_text(const bqsr_sam* s, char* dst, int64_t cap, int64_t* len);

/* BAM records (SAM spec §4.2, little endian) of records [r0, r0 + n) of the
 * parse, from its current text (after bqsr_sam_rewrite_quals / bqsr_sam_sort:
 * QUAL and FLAG final; a BAM-born parse holds SAM lines too), its CIGAR
 * words and its @SQ index, encoded on the device.  Per record, block_size
 * first:
 *   refID        the @SQ index of RNAME ("*": -1)
 *   pos          POS - 1
 *   l_read_name  QNAME length + 1
 *   mapq         as given
 *   bin          the spec's reg2bin(pos, end), arithmetic shifts; end = pos +
 *                the CIGAR's reference length (M D N = X), pos + 1 when that
 *                is 0 or CIGAR is "*" (so pos = -1 gives 4680)
 *   n_cigar_op   the parse's CIGAR element count
 *   flag         as given (0x400 following MarkDuplicates when it ran)
 *   l_seq        SEQ length, 0 for "*"
 *   next_refID   "=": refID; "*": -1
 *   next_pos     PNEXT - 1
 *   tlen         as given
 *   read_name    QNAME, NUL
 *   cigar        the parse's u32 words (len << 4 | op), none for "*"
 *   seq          4-bit codes of "=ACMGRSVTWYHKDBN", upper-cased, anything else
 *                15, high nibble first
 *   qual         each byte - 33; l_seq bytes of 0xFF for "*"
 *   tags, in input order: A; i as the smallest of c C s S i I that holds the
 *                value, the signed type when both fit; f as binary32 (what C
 *                strtof gives for the text: the slots are filled on the host
 *                before the bytes are handed out); Z and H as the bytes and a
 *                NUL; B:t,v,... for t in cCsSiIf as the type byte, an int32
 *                count and the values ("B:c" alone: count 0).
 * BQSR_ERR_UNSUPPORTED, with the first offending read in input order
 * (bqsr_last_error_read) and nothing written, for what BAM cannot hold or
 * the spec forbids: RNAME / RNEXT that is neither "*" (nor "=") nor an @SQ
 * name; QNAME above 254 bytes; more than 65535 CIGAR elements; POS - 1 /
 * PNEXT - 1 / TLEN outside int32; FLAG outside 16 bits, MAPQ outside 8; a
 * QUAL other than "*" whose byte length differs from SEQ's or with a byte
 * outside '!'..'~' (the reference's trimmed recalibrated strings and its
 * chars above 0x7F, which the SAM text sink keeps writing); an unknown tag
 * type letter; an 'i' value outside [-2^31, 2^32 - 1]; a B value outside its
 * element type; an odd-length or non-hex H; a value that is not of its type.
 * prepare: pass 1 (the checks, every record's size) and the byte count;
 * records: pass 2 and the copy into dst (sizes.bytes bytes of host memory),
 * floats final. */
typedef struct bqsr_bam_sizes {
  int64_t n_reads;
  int64_t bytes;    /* of the records, block_size words included */
  int64_t n_floats; /* f values (tags and B:f elements) converted on the host */
} bqsr_bam_sizes;
bqsr_status bqsr_sam_bam_prepare(bqsr_context* ctx, bqsr_sam* s, int64_t r0, int64_t n, void* stream,
                                 bqsr_bam_sizes* out);
bqsr_status bqsr_sam_bam_records(bqsr_context* ctx, bqsr_sam* s, uint8_t* dst, void* stream);
/* The BAM header of the parse: "BAM\1", l_text, the header text unchanged (no
 * SO: edit, as bqsr_sam_sort), n_ref, and every @SQ line in order as l_name,
 * name, NUL, LN (0 when absent).  *len: its size; at most cap bytes are
 * copied (dst NULL with cap 0: the size only). */
bqsr_status bqsr_sam_bam_header(const bqsr_sam* s, uint8_t* dst, int64_t cap, int64_t* len);
/* BGZF members of a byte stream (SAM spec §4.1), by min(16, hardware
 * threads) host threads: `in` cut into members of 65280 bytes (a record may
 * straddle two), each raw DEFLATE at `level` (1-9: libdeflate, zlib at
 * windowBits -15 when absent; 0, or a member DEFLATE would not shrink: one
 * stored block) with BSIZE in the BC extra field, CRC32 and ISIZE.  No EOF
 * member: the caller appends the 28-byte marker once.  *out_len: the size,
 * also when it exceeds cap (BQSR_ERR_INVALID_ARG then); n + 64 * (n / 65280
 * + 1) bytes always suffice.  No device call. */
bqsr_status bqsr_bgzf_compress(const uint8_t* in, int64_t n, int32_t level, uint8_t* out, int64_t cap,
                               int64_t* out_len);
/* MEASUREMENT ONLY, not part of the stable interface: the device-event times
 * of the calling thread's last bqsr_sam_bam_prepare (pass 1) and
 * bqsr_sam_bam_records (pass 2) kernels, in milliseconds
 * (tools/bench_adam.py --bam-out). */
bqsr_status bqsr_bam_kernel_times(double* len_ms, double* write_ms);
/* BGZF members deflated on the device (bgzf_deflate.hip), the inverse of
 * bqsr_bgzf_inflate: `in` (host memory) is uploaded, cut as bqsr_bgzf_compress
 * cuts it (members of 65280 bytes, the last one short, none for n == 0, no
 * EOF member) and every member compressed by one workgroup: LZ77 matches
 * within the member only (distance <= 32768, length 3..258, runs included),
 * a greedy parse, and the smallest of one dynamic-Huffman block, one
 * fixed-Huffman block and one stored block (a member DEFLATE would not shrink
 * is stored: 31 bytes more than its data); BSIZE in the BC field, CRC32 and
 * ISIZE computed on the device.  The members are packed there and only the
 * packed bytes come back.  The bytes are a function of the input alone (no
 * level, no dependence on timing).  *out_len: the size, also when it exceeds
 * cap (BQSR_ERR_INVALID_ARG then); n + 64 * (n / 65280 + 1) bytes always
 * suffice.  *n_members (may be NULL): the members written. */
bqsr_status bqsr_bgzf_deflate(bqsr_context* ctx, const uint8_t* in, int64_t n, void* stream, uint8_t* out, int64_t cap,
                              int64_t* out_len, int64_t* n_members);
/* The same member routine compiled for the host, a lane at a time: the bytes
 * bqsr_bgzf_deflate gives, without a device call.  For tests on a machine
 * without a GPU; far slower than bqsr_bgzf_compress. */
bqsr_status bqsr_bgzf_deflate_host(const uint8_t* in, int64_t n, uint8_t* out, int64_t cap, int64_t* out_len,
                                   int64_t* n_members);
/* After bqsr_sam_bam_prepare, in place of bqsr_sam_bam_records: pass 2 into
 * the device buffer, the float tags' values converted on the host as there
 * (only the patch list and the texts are downloaded) and scattered into the
 * device stream, then that stream deflated as bqsr_bgzf_deflate does it.  dst
 * receives the members, which inflate to exactly the bytes
 * bqsr_sam_bam_records hands out.  *out_len also when it exceeds cap
 * (BQSR_ERR_INVALID_ARG); sizes.bytes + 64 * (sizes.bytes / 65280 + 1) bytes
 * always suffice.  BQSR_ERR_INVALID_ARG when the text changed since the
 * prepare. */
bqsr_status bqsr_sam_bam_members(bqsr_context* ctx, bqsr_sam* s, void* stream, uint8_t* dst, int64_t cap,
                                 int64_t* out_len);
/* Host only, no device call: the code lengths the encoder gives a histogram
 * (deflate_codes.h, the routine the kernel runs).  len_out[i]: 0 for
 * freq[i] == 0, otherwise 1..max_bits; a single used symbol gets 1; with two
 * or more the lengths form a complete code (Kraft sum 1), and where the plain
 * Huffman code fits max_bits their cost is Huffman's.  BQSR_ERR_INVALID_ARG
 * when n_syms > 2^max_bits or max_bits is outside 1..15. */
bqsr_status bqsr_deflate_code_lengths(const uint32_t* freq, int32_t n_syms, int32_t max_bits, uint8_t* len_out);
/* MEASUREMENT ONLY, not part of the stable interface: the device-event times
 * of the calling thread's last device deflate (bqsr_bgzf_deflate or
 * bqsr_sam_bam_members): the member kernel and the pack kernel, in
 * milliseconds. */
bqsr_status bqsr_bgzf_deflate_times(double* deflate_ms, double* pack_ms);

/* The .bai index of a BAM while it is written (`transform OUT.bam -bam_index`;
 * SAM spec §5.2, bam_index.hip): one object across the pieces and partitions
 * of one output, fed from the device buffers of every bqsr_sam_bam_prepare.
 * No htslib is consulted; the index is the spec plus these declarations.
 *
 * Interval of a record.  [beg, end) is the interval the record's bin field
 *   comes from (bqsr_sam_bam_prepare above: beg = POS - 1, end = beg + the
 *   CIGAR's reference length over M D N = X, beg + 1 when that is 0 or CIGAR
 *   is "*"; one routine computes both).  For the index a negative beg (POS 0
 *   with an RNAME) is clamped to 0 and end is at least beg + 1; the order
 *   checks below use the clamped beg.  A record with refID >= 0 is indexed
 *   whether or not FLAG 0x4 is set.
 * Virtual offsets.  The record stream is the BAM header followed by every
 *   record; position p lies in the BGZF member m with start[m] <= p <
 *   start[m + 1] and its virtual offset is file_offset[m] << 16 | (p -
 *   start[m]).  A record's u is the offset of its block_size word, its v that
 *   of the position one past its last byte: when that falls on a member
 *   boundary it is expressed in the next member with offset 0, for the last
 *   record of the file in the EOF marker.  A piece ends in a short member, so
 *   the caller builds the member table from the BSIZE and ISIZE fields of the
 *   bytes it writes (header members, every piece, the EOF marker) and hands it
 *   over as (stream start, file offset) per member plus a terminal entry (the
 *   stream's length, the file's size).
 * Binning index.  bin = reg2bin(beg, end).  Within one (refID, bin) records
 *   are taken in file order; a record joins the chunk before it when prev.v
 *   >> 16 >= u >> 16 (prev: the record before it in the bin) and the chunk's
 *   end becomes the record's v, otherwise it starts a chunk.  Bins ascend by
 *   number; small bins are not folded into their parents.
 * Pseudo-bin 37450, last for every reference with records and counted in
 *   n_bin: chunk (u of the reference's first record, v of its last), chunk
 *   (records without FLAG 0x4, records with it); FLAG is the one written
 *   (after MarkDuplicates), not BQSR_F_MAPPED.
 * Linear index.  n_intv = 1 + ((max end - 1) >> 14) over the reference's
 *   records; window w holds the smallest u among records with beg >> 14 <= w
 *   <= (end - 1) >> 14; an empty window takes the value of the window before
 *   it, empty windows before the first filled one hold 0.
 * A reference without records has n_bin = 0 and n_intv = 0.  n_no_coor, the
 *   number of records with refID -1, is always written.
 * Refusals at bqsr_bam_index_finish, each naming the first offending record
 *   by its ordinal in the whole output (bqsr_last_error_read); when one record
 *   earns both, the first one listed:
 *   BQSR_ERR_UNSORTED     among records with refID >= 0 the refID decreases or
 *                         beg decreases inside one reference, or such a record
 *                         follows one with refID -1.  (bqsr_sam_sort puts
 *                         every read with FLAG 0x4 after the mapped ones: its
 *                         output is refused when such a read has an RNAME.)
 *   BQSR_ERR_UNSUPPORTED  end > 2^29, BAI's limit; more than 2^32 - 1 records
 *                         (at bqsr_bam_index_add).
 * Device memory: 24 bytes per record from the add on; during finish 56 more
 * per record (80 in all), 16 per chunk, 12 per bin, 8 per window, and
 * rocprim's workspace.  What does not fit is BQSR_ERR_UNSUPPORTED.
 *
 * create (n_ref: the BAM header's reference count); add after every
 * bqsr_sam_bam_prepare of the output, in output order (stream_base: the
 * stream position of the piece's first byte; one kernel, nothing downloaded);
 * set_members ([2 (n_members + 1)] uint64: the table above, terminal entry
 * last); finish (the work listed in bam_index.hip; only the chunks, bins,
 * windows and per-reference words come back); size and bytes (the file);
 * destroy. */
typedef struct bqsr_bam_index bqsr_bam_index;
typedef struct bqsr_bam_index_sizes {
  int64_t n_records;
  int64_t n_chunks;     /* pseudo-bins' not counted */
  int64_t n_bins;       /* pseudo-bins not counted */
  int64_t n_windows;
  int64_t bytes;        /* of the .bai file */
  int64_t device_bytes; /* held on the device when finish returned */
} bqsr_bam_index_sizes;
bqsr_status bqsr_bam_index_create(bqsr_context* ctx, int32_t n_ref, bqsr_bam_index** out);
void bqsr_bam_index_destroy(bqsr_bam_index* x);
bqsr_status bqsr_bam_index_add(bqsr_bam_index* x, bqsr_sam* s, int64_t stream_base, void* stream);
bqsr_status bqsr_bam_index_set_members(bqsr_bam_index* x, const uint64_t* members, int64_t n_members, void* stream);
bqsr_status bqsr_bam_index_finish(bqsr_bam_index* x, void* stream);
bqsr_status bqsr_bam_index_size(const bqsr_bam_index* x, bqsr_bam_index_sizes* out);
bqsr_status bqsr_bam_index_bytes(const bqsr_bam_index* x, uint8_t* dst, int64_t cap);
/* MEASUREMENT ONLY, not part of the stable interface: ms6 receives the stages
 * of this index in transform.BAM_INDEX_KERNELS' order, in milliseconds: the
 * rows kernels of every add, locate, windows, sort and chunks by device
 * events, the serialisation by the host clock. */
bqsr_status bqsr_bam_index_kernel_times(const bqsr_bam_index* x, double* ms6);

/* A BAM read in windows (bam_windows.hip): what `python -m adam_amd.bam_index`
 * (the index of a BAM some other tool wrote) and `-region` (a read through a
 * .bai index) share.  `bam` is the whole file in host memory (a read-only map);
 * it must outlive the reader.  Device memory is bounded by the window.
 *
 * Members.  open walks the file's BSIZE / ISIZE fields (every member, empty
 *   ones and the EOF marker included): bqsr_bam_reader_members hands out the
 *   table bqsr_bam_index_set_members takes, [2 (n_members + 1)] uint64 of
 *   (stream start, file offset) and the terminal (stream length, file size).
 * Window.  A run of whole members, inflated on the device with the kernels of
 *   bqsr_bgzf_inflate; a member those decline is inflated by the host, and one
 *   the host declines too is BQSR_ERR_SAM_PARSE.  A window starts at the member
 *   that holds the next record's first byte and takes members while it stays
 *   within piece_bytes of inflated stream (1 .. 2^31) and before end_member
 *   (at least one member); when it holds no whole record from its start it is
 *   extended, member by member, to what that record's block_size asks for,
 *   whatever piece_bytes and end_member say; a block_size that points past
 *   the stream's end is the "truncated record" refusal at once, with nothing
 *   more inflated.  The members the host inflated are counted (members_host),
 *   and a parse that holds one reports bqsr_sam_bam_form 1, else 2.
 * Walk.  The offsets of the window's complete records are found from the
 *   known offset of the first: the header's end for the first window, where the
 *   window before stopped for a later one, what bqsr_bam_reader_seek named for
 *   a region read.  The device chain is bqsr_bam_parse's (a guess per member,
 *   a check that every walk lands on the next guess, the offsets written at
 *   scanned counts) with two changes: the first member's start is the given
 *   one, and the last walk may leave the window: the record it cannot finish
 *   is not taken, and the next window starts at the member that holds its
 *   first byte.  Where the check declines, the window's bytes are walked by the
 *   host (bqsr_bam_window.device = 0; the stats count both forms).
 * Header.  Magic, text and reference list are read by open from windows of the
 *   file's first members (they are not counted as members read).
 * Refusals, BQSR_ERR_SAM_PARSE: not BGZF, a member cut by the file's end, no
 *   BAM magic, a member that does not inflate, a block_size below 32, a record
 *   whose name and CIGAR do not fit its block_size, a record the file's end
 *   cuts ("truncated record").  Those about a record name it by its ordinal
 *   among the records seen (bqsr_last_error_read): the ordinal in the file for
 *   a read from the header's end on.
 *
 * open; then next until .done (n_records may be 0 only with .done); after each
 * next, the window's records go to an index (bqsr_bam_index_add_window: a row
 * each, with the interval rule stated at bqsr_bam_index_create, from refID, pos,
 * FLAG and the CIGAR words of the raw record) or through the region filter:
 * bqsr_bam_reader_filter keeps, a lane per record, those with refID == ref, beg
 * < end and end > beg in that interval (so a placed read with FLAG 0x4 is
 * kept) that start before stream position `limit` (a chunk's v; a malformed
 * record at or past it is not this read's to refuse); the kept
 * records are compacted by a scan and a copy (a wavefront stores its 64
 * records' bytes contiguously) into one device buffer that lives across
 * windows.  *done: 1 when a record at or past `limit` was seen (the chunk is
 * over), 2 when a record of a later reference, without one, or with beg >= end
 * was seen: in a sorted file nothing after it overlaps, and nothing after it is
 * kept.  bqsr_bam_reader_seek (member index, offset inside its inflated bytes)
 * sets where the next window's first record starts.  bqsr_bam_reader_parse
 * turns the kept records into a bqsr_sam as bqsr_bam_parse does for a whole
 * file (the same lines kernels and parse): header plus kept records in the
 * order they were kept. */
typedef struct bqsr_bam_reader bqsr_bam_reader;
typedef struct bqsr_bam_window {
  int64_t n_records;     /* complete records found in this window */
  int64_t member_begin;  /* the window's members [member_begin, member_end) */
  int64_t member_end;
  int64_t next_pos;      /* stream position of the next record */
  int32_t device;        /* 1: the device chain; 0: the host's walk */
  int32_t done;          /* the stream's end is reached */
} bqsr_bam_window;
typedef struct bqsr_bam_reader_stats {
  int64_t members_total, stream_bytes, n_ref, body;
  int64_t members_read, windows_device, windows_host, records_seen, records_kept;
  int64_t members_host;  /* members the kernels declined and the host inflated (the header's windows included) */
  double filter_ms;      /* region filter, scan and copy, by device events */
} bqsr_bam_reader_stats;
bqsr_status bqsr_bam_reader_open(bqsr_context* ctx, const uint8_t* bam, int64_t n_bytes, int64_t piece_bytes,
                                 void* stream, bqsr_bam_reader** out);
void bqsr_bam_reader_destroy(bqsr_bam_reader* r);
bqsr_status bqsr_bam_reader_members(const bqsr_bam_reader* r, uint64_t* members, int64_t cap);
bqsr_status bqsr_bam_reader_seek(bqsr_bam_reader* r, int64_t member, int64_t offset);
bqsr_status bqsr_bam_reader_next(bqsr_bam_reader* r, int64_t end_member, void* stream, bqsr_bam_window* out);
bqsr_status bqsr_bam_index_add_window(bqsr_bam_index* x, bqsr_bam_reader* r, void* stream);
bqsr_status bqsr_bam_reader_filter(bqsr_bam_reader* r, int32_t ref, int64_t beg, int64_t end, int64_t limit,
                                   void* stream, int64_t* kept, int32_t* done);
bqsr_status bqsr_bam_reader_parse(bqsr_bam_reader* r, void* stream, bqsr_sam** out);
bqsr_status bqsr_bam_reader_get_stats(const bqsr_bam_reader* r, bqsr_bam_reader_stats* out);

/* MarkDuplicates (§8 f3): adam-core/.../rdd/MarkDuplicates.scala:24-111 over
 * SingleReadBucket (models/SingleReadBucket.scala:27-37: reads grouped by
 * (recordGroupId, readName)) and ReferencePositionPair
 * (models/ReferencePositionPair.scala:27-63: the buckets' 5' positions,
 * RichADAMRecord.scala:77-118).  Buckets grouped by (left position,
 * library), then by right position; the best-scoring bucket of a group
 * (score = Σ quals >= 15 of its primary reads, :37-39) keeps its primary
 * reads, every other mapped read of the group is a duplicate, unmapped reads
 * never are.  Ties go to the bucket seen first (Spark leaves their order to
 * its shuffle).  Host C++: a grouping step in front of the device passes. */
typedef struct bqsr_dup_reads {
  int64_t n_reads;
  const char* const* read_name; /* [n] readName (NULL = null)                      */
  const char* const* library;   /* [n] recordGroupLibrary (NULL = null)            */
  const uint32_t* flags;        /* [n] BQSR_F_* (PAIRED, MAPPED, NEG_STRAND, PRIMARY, HAS_RG) */
  const uint8_t* mate_mapped;   /* [n] mateMapped                                  */
  const int32_t* rg_id;         /* [n] recordGroupId (when BQSR_F_HAS_RG)          */
  const int32_t* reference_id;  /* [n] referenceId                                 */
  const int64_t* start;         /* [n] 0-based start                               */
  const uint64_t* qual_offset;  /* [n+1] */
  const uint8_t* qual;          /* phred+33 chars                                  */
  const uint64_t* cigar_offset; /* [n+1] */
  const uint32_t* cigar;        /* BAM-encoded elements                            */
} bqsr_dup_reads;
/* dup[r] = the duplicateRead value MarkDuplicates gives read r */
bqsr_status bqsr_mark_duplicates(const bqsr_dup_reads* reads, uint8_t* dup);
/* The same over a parse (readName = QNAME, referenceId = the @SQ index,
 * mateMapped from FLAG 0x8, library = the read group's LB); the parse's
 * flags column gets BQSR_F_DUPLICATE set or cleared accordingly, as
 * `transform -mark_duplicate_reads` does before BQSR.
 * Runs on the device.  Its packed keys hold 32767 contigs (referenceId, the
 * @SQ index, 0..32766) and 4095 distinct LB values among the header's read
 * groups: a primary mapped read on a later contig, or a bucket whose library
 * is the 4096th or later in sorted order, makes this call redo the work with
 * the host form (the same result, slower); so does a 64-bit collision of the
 * bucket hash.  bqsr_sam_markdup_path tells which ran. */
bqsr_status bqsr_sam_mark_duplicates(bqsr_sam* s, int64_t* n_duplicates);
/* Which path served the last bqsr_sam_mark_duplicates on this parse: -1 not
 * run (or it failed), 0 the device, otherwise a bit mask of why the host form
 * did it: 1 a hash collision between two buckets, 2 a contig or a position
 * beyond the packed key, 4 a library rank of 4096 or more, 8 forced
 * (ADAM_BQSR_MARKDUP=host, or 2^31 - 1 reads or more). */
int bqsr_sam_markdup_path(const bqsr_sam* s);

/* Sort by reference position (`transform -sort_reads`):
 * adamSortReadsByReferencePosition (adam-core/.../rdd/AdamRDDFunctions.scala:63-93)
 * with ReferencePosition's ordering (models/ReferencePosition.scala:73-95,
 * 155-166: referenceId, then pos), the last step of Transform.run
 * (adam-cli/.../cli/Transform.scala:89-93), after MarkDuplicates and BQSR.
 *   mapped reads (readMapped, the BQSR_F_MAPPED bit: FLAG non-zero (Q2)
 *     without 0x4): key (referenceId, start); referenceId is the @SQ index.
 *     A mapped read whose referenceId or start is null (RNAME "*" or not in
 *     @SQ, POS 0) makes the reference throw a NullPointerException
 *     (mappedPositionCheck wraps both in Some(...), the constructor unboxes
 *     null): BQSR_ERR_NULL_FIELD naming the first such read in input order
 *     (bqsr_last_error_read), the parse left unchanged.
 *   every other read: key (Int.MaxValue - c, Long.MaxValue), c = n mod 10001
 *     with n the read's 1-based ordinal among the unmapped reads of its
 *     partition (the iterator at :70-82 counts 1 .. 10000, then 0).  They
 *     follow all mapped reads in descending c: up to 10000 of them in the
 *     reverse of their input order; 10002 come out as 10000, 9999, .., 1,
 *     10002, 10001.  The whole input is one partition.
 *   equal keys keep their input order (a stable sort: what the reference
 *     gives on one partition; Spark leaves it to the shuffle otherwise).
 * BQSR_ERR_UNSUPPORTED for what the packed 64-bit key cannot order: a
 * negative referenceId or start, a start >= 2^32 - 1, a mapped referenceId >=
 * Int.MaxValue - 10000, more than 2^32 - 1 reads.
 *
 * order[i] = input index of the read at sorted position i (device, [n]);
 * flags' BQSR_F_MAPPED bit, reference_id / start with nulls marked as the
 * parse's columns mark them (reference_id -1; start without
 * BQSR_F_HAS_START in flags); device pointers */
bqsr_status bqsr_sort_order(bqsr_context* ctx, int64_t n, const uint32_t* flags, const int32_t* reference_id,
                            const int64_t* start, uint32_t* order, void* stream);
/* the parse's records reordered as above: the new text is the header bytes
 * unchanged (no "SO:coordinate": this is not samtools' coordinate order),
 * then the records as bqsr_sam_rewrite_quals(b = NULL) emits them, in
 * sorted order; the handle is then what bqsr_sam_parse of that text gives
 * (columns, counts, referenceNames in first-appearance order, ADAM columns),
 * with MarkDuplicates' result carried along.  BQSR_ERR_INVALID_ARG while a
 * bqsr_sam_adam_set_quals is pending (its batch is in the old order: rewrite
 * the text first).  Peak device memory: twice the text, and the new columns
 * beside the old ones while the records are parsed again. */
bqsr_status bqsr_sam_sort(bqsr_context* ctx, bqsr_sam* s, void* stream);

/* `adam flagstat` (adam-cli/.../cli/FlagStat.scala:43-109 over adamFlagStat,
 * adam-core/.../rdd/FlagStat.scala:21-116): eighteen counters, kept once for
 * the reads with failedVendorQualityChecks false (`passed`) and once for true
 * (`failed`), in FlagStatMetrics' order (the BQSR_FS_* indices).  Per record,
 * with the ADAMRecord fields as SAMRecordConverter.scala:26-108 sets them
 * (every boolean false when FLAG is 0; the pair booleans only with 0x1;
 * referenceId / mapq only when RNAME is an @SQ name, mapq only when MAPQ !=
 * 255; mateReferenceId only when RNEXT resolves, "=" being RNAME's id):
 *   dup = duplicateRead && primaryAlignment (primary) / && !primaryAlignment
 *     (secondary); for either: dup; dup && readMapped && mateMapped; dup &&
 *     readMapped && !mateMapped; dup && referenceId != mateReferenceId -- not
 *     gated by readPaired.  The inequality is Scala's on boxed Integers: null
 *     equals null, null differs from a value (an unpaired duplicate with RNAME
 *     set and RNEXT "*" counts as cross chromosome).
 *   mapped = readMapped; pairedInSequencing = readPaired; read1 / read2 /
 *     properlyPaired = readPaired && firstOfPair / secondOfPair / properPair;
 *     withSelfAndMateMapped / singleton = readPaired && readMapped &&
 *     mateMapped / !mateMapped; withMateMappedToDiffChromosome = readPaired &&
 *     readMapped && mateMapped && referenceId != mateReferenceId; ...MapQ5 =
 *     that && mapq >= 5.  Where that holds and mapq is null the reference
 *     unboxes null and throws: BQSR_ERR_NULL_FIELD naming the first such read
 *     in input order (bqsr_last_error_read), `out` zeroed.
 * `out` holds the counts of this call only; callers add results (the
 * reference's `+`).  Device: one reduction kernel per front end
 * (adam_amd/csrc/flagstat.hip), integer sums (independent of launch order). */
enum {
  BQSR_FS_TOTAL = 0,
  BQSR_FS_DUP_PRIMARY = 1,   /* total, bothMapped, onlyReadMapped, crossChromosome */
  BQSR_FS_DUP_SECONDARY = 5, /* the same four */
  BQSR_FS_MAPPED = 9,
  BQSR_FS_PAIRED_IN_SEQUENCING = 10,
  BQSR_FS_READ1 = 11,
  BQSR_FS_READ2 = 12,
  BQSR_FS_PROPERLY_PAIRED = 13,
  BQSR_FS_WITH_SELF_AND_MATE_MAPPED = 14,
  BQSR_FS_SINGLETON = 15,
  BQSR_FS_MATE_DIFF_CHROMOSOME = 16,
  BQSR_FS_MATE_DIFF_CHROMOSOME_MAPQ5 = 17,
  BQSR_FS_COUNTERS = 18
};
typedef struct bqsr_flagstat_metrics {
  int64_t c[18];
} bqsr_flagstat_metrics;
typedef struct bqsr_flagstat {
  bqsr_flagstat_metrics passed, failed;
} bqsr_flagstat;
/* over a parse (SAM or BAM): FLAG and referenceId from the parse's columns,
 * MAPQ and RNEXT from each read's line; duplicateRead is the flags column's
 * bit, so after bqsr_sam_mark_duplicates the counts follow its result, not
 * the input's 0x400 */
bqsr_status bqsr_sam_flagstat(bqsr_context* ctx, const bqsr_sam* s, void* stream, bqsr_flagstat* out);
/* over Arrow buffers (ADAMRecord Parquet as Arrow decodes it): host pointers,
 * uploaded as they are, one chunk per record batch (array offsets 0; chunk
 * lengths need not be multiples of 64).  bools: readPaired, properPair,
 * readMapped, mateMapped, firstOfPair, secondOfPair, primaryAlignment,
 * duplicateRead, failedVendorQualityChecks as Arrow bitmaps (LSB first).  A
 * NULL boolean column is all false, a NULL validity bitmap all valid, a NULL
 * int column all null; a null boolean reads as false (as bqsr_arrow_chunk).
 * Only ceil(n_reads / 8) bytes of a bitmap are read, and bits at and beyond
 * n_reads are not counted.  NULL_FIELD's read index is global over the
 * chunks. */
typedef struct bqsr_flagstat_chunk {
  int64_t n_reads;
  const uint8_t* bools[9];
  const uint8_t* bools_validity[9];
  const int32_t* reference_id;
  const uint8_t* reference_id_validity;
  const int32_t* mate_reference_id;
  const uint8_t* mate_reference_id_validity;
  const int32_t* mapq;
  const uint8_t* mapq_validity;
} bqsr_flagstat_chunk;
bqsr_status bqsr_flagstat_arrow(bqsr_context* ctx, const bqsr_flagstat_chunk* chunks, int32_t n_chunks, void* stream,
                                bqsr_flagstat* out);
/* MEASUREMENT ONLY, not part of the stable interface (it may change or go
 * without notice; callers use bqsr_flagstat_arrow): the Arrow-form kernel
 * alone, enqueued on `stream`, so that tools/bench_adam.py --flagstat can time
 * it with device events.  Nothing is checked: every pointer of `chunk` must be
 * device memory, the bitmaps padded to whole 64-bit words and 8-byte aligned;
 * `counters` = 37 device words the sums are added into (passed[18],
 * failed[18], then the first NULL_FIELD read, to be preset to all ones). */
bqsr_status bqsr_flagstat_arrow_device(bqsr_context* ctx, const bqsr_flagstat_chunk* chunk, void* counters,
                                       void* stream);

/* `adam print_tags` (adam-cli/.../cli/PrintTags.scala:35-91 over
 * adamCharacterizeTags / adamCharacterizeTagValues, adam-core/.../rdd/
 * AdamRDDFunctions.scala:200-229, RichADAMRecord.tags, .../rich/
 * RichADAMRecord.scala:46, and AttributeUtils, .../util/AttributeUtils.scala:
 * 28-99): how often each two-char tag occurs among the attributes of the
 * records with failedVendorQualityChecks false, how many such records there
 * are, and -- a tag a call -- the distinct values of a tag with their counts.
 *
 * Rules (adam_amd/csrc/tags.hip):
 *   - a record's attributes are its string split on tabs, empty pieces dropped;
 *     every piece must match ([^:]{2}):([AifZHB]):(.*) as a whole (Java's `.`
 *     stops at \n, \r, U+0085, U+2028, U+2029) and its value must convert: A a
 *     first char, i Integer.valueOf, f Float.valueOf, H decimal digits only, B
 *     comma-separated Float.valueOf (pieces with '.') / Integer.valueOf.  What
 *     the reference throws at is BQSR_ERR_ATTRIBUTE.  Values are converted for
 *     every attribute of every kept record, counted or not.
 *   - a tag byte >= 0x80, or one inside an A / i / f / H / B value, is
 *     BQSR_ERR_UNSUPPORTED (Z values may hold any bytes).
 *   - a null failedVendorQualityChecks, or null attributes on a kept record, is
 *     BQSR_ERR_NULL_FIELD (the reference unboxes / dereferences null).
 *   - over a parse, a record's attributes are what SAMRecordConverter builds
 *     (bqsr_sam_adam_*: htsjdk's tag list, a repeated tag replaced by its later
 *     value, MD left out), and a record the converter cannot convert fails the
 *     call with what bqsr_sam_adam_prepare returns for it -- kept or not.  At
 *     most 48 tags a record.  Kept = FLAG 0x200 clear.
 *   - over Arrow buffers every occurrence of a tag counts; the value of a
 *     record under bqsr_arrow_tag_values is that of its first attribute with
 *     the tag, over a parse that of the surviving one.
 *   - the first failing record in input order is reported
 *     (bqsr_last_error_read; global over the chunks).  Within a record:
 *     conversion errors, then NULL_FIELD, then the first bad attribute in
 *     string order.
 * counts[b0 * 128 + b1] is the count of the tag with bytes b0, b1.  `out`
 * holds the results of this call only; callers add them.  Integer sums,
 * independent of launch order. */
typedef struct bqsr_tag_counts {
  int64_t counts[128 * 128];
  int64_t total; /* the kept records */
} bqsr_tag_counts;
/* one Arrow record batch, host pointers uploaded as they are: `attributes` as
 * Arrow string (int32 offsets [n_reads + 1], bytes, validity) and the
 * failedVendorQualityChecks bitmap with its validity (LSB first).  Array
 * offsets 0; attr_offsets[0] need not be 0.  Bitmaps are read to
 * ceil(n_reads / 8) bytes.  A NULL validity is all valid; NULL attr_offsets is
 * a column of nulls, NULL failed a column of nulls. */
typedef struct bqsr_tags_chunk {
  int64_t n_reads;
  const int32_t* attr_offsets;
  const uint8_t* attr_bytes;
  const uint8_t* attr_validity;
  const uint8_t* failed;
  const uint8_t* failed_validity;
} bqsr_tags_chunk;
bqsr_status bqsr_sam_tag_counts(bqsr_context* ctx, const bqsr_sam* s, void* stream, bqsr_tag_counts* out);
bqsr_status bqsr_arrow_tag_counts(bqsr_context* ctx, const bqsr_tags_chunk* chunks, int32_t n_chunks, void* stream,
                                  bqsr_tag_counts* out);
/* The values of tag (two bytes) as runs: (type letter of A i f Z H, count,
 * first record in input order, value text -- the char, the decimal int,
 * Float.toString, or the bytes of a Z / H value).  Two runs may carry the same
 * (type, text): callers merge them, and the results of several calls.  Values
 * are grouped by a 64-bit key (type, then the scalar or a hash of the bytes cut
 * to hash_bits, 1..64; 64 in normal use, fewer to force collisions in tests);
 * equal keys with different bytes make different runs.  A value of type B is
 * BQSR_ERR_UNSUPPORTED (the reference keys the array by identity).  The values
 * calls do not validate: run the counts call over the same records first.
 * prepare / fetch: the sizes of the calling thread's last values call, then
 * bqsr_tag_values_fetch into buffers of n_runs (text_offsets: n_runs + 1) and
 * text_bytes elements. */
typedef struct bqsr_tag_value_sizes {
  int64_t n_runs, text_bytes;
} bqsr_tag_value_sizes;
typedef struct bqsr_tag_value_host {
  uint8_t* type;
  int64_t* count;
  int64_t* first_read;
  int64_t* text_offsets;
  uint8_t* text;
} bqsr_tag_value_host;
bqsr_status bqsr_sam_tag_values(bqsr_context* ctx, const bqsr_sam* s, const char* tag, int32_t hash_bits,
                                void* stream, bqsr_tag_value_sizes* out);
bqsr_status bqsr_arrow_tag_values(bqsr_context* ctx, const bqsr_tags_chunk* chunks, int32_t n_chunks, const char* tag,
                                  int32_t hash_bits, void* stream, bqsr_tag_value_sizes* out);
bqsr_status bqsr_tag_values_fetch(const bqsr_tag_value_host* dst);
/* MEASUREMENT ONLY, not part of the stable interface: device-event times of
 * the calling thread's last counts call (the scan kernels) and last values
 * call (the value kernels with their sorts and scans), in ms */
bqsr_status bqsr_tags_kernel_times(double* scan_ms, double* values_ms);

/* `adam reads2ref` (adam-cli/.../cli/Reads2Ref.scala:53-75 over
 * Reads2PileupProcessor.readToPileups, adam-core/.../rdd/Reads2PileupProcessor.
 * scala:34-197): reads [r0, r0 + n) of a parse as ADAMPileup rows
 * (adam-format/.../avro/adam.avdl:99-128), one per M, I, D or S base of the
 * read's CIGAR; N, H, P, = and X elements produce none.  Reads in input
 * order; a read's rows in REVERSE walk order (the reference prepends).
 *   A read without CIGAR or without MD (no MD:Z tag) gives no rows.  Otherwise
 *   a null start is BQSR_ERR_NULL_FIELD, an MD tag MdTag.apply rejects
 *   BQSR_ERR_MD_PARSE (MdTag.scala:38-98; "" is the empty tag), and the walk
 *   starts with referencePos = start, readPos = 0; the MD is looked up at
 *   referencePos - start, also after an N (which the MD does not count: the
 *   reference looks in the wrong place, and so does this).
 *     M  referenceBase = the read's base where the MD says match, else the
 *        MD's mismatch base; readBase; rangeOffset / rangeLength null
 *     I  readBase; rangeOffset = index in the element, rangeLength = its
 *        length; referenceBase null; position = the unchanged referencePos
 *     D  referenceBase = the MD's deleted base; readBase null; range as I;
 *        sangerQuality from the NEXT read base (a trailing D throws)
 *     S  as I, and numSoftClipped = 1
 *   every row: position, sangerQuality = (int)(signed byte)(qual - 33),
 *   mapQuality = mapq (nullable), numReverseStrand = readNegativeStrand,
 *   readStart = start, readEnd = start + the reference-consuming lengths.
 *   BQSR_ERR_PILEUP where the walk throws: a sequence char outside the Base
 *   enum ("*", "=", ".", lower case: the MD is upper-cased, the sequence is
 *   not); sequence or quals shorter than the CIGAR's read bases; an M base
 *   the MD has as a delete or not at all; a D base the MD has no delete for;
 *   a read with readMapped false that would give a row (record.end is None) --
 *   which, with quirk Q2, includes every FLAG-0 SAM record with CIGAR and MD.
 *   A null sequence or qual reached by the walk is BQSR_ERR_NULL_FIELD.  The
 *   first exception in the reference's evaluation order decides a read's
 *   status; the first throwing read in input order decides the call's
 *   (bqsr_last_error_read; no rows).
 *   Nothing is filtered here: LocusPredicate applies to Parquet input only
 *   (AdamContext.scala:318-332) and is the caller's (adam_amd/reads2ref.py).
 *   The flags column is used as it stands and only readMapped and
 *   readNegativeStrand are read, so bqsr_sam_mark_duplicates changes nothing.
 * BQSR_ERR_UNSUPPORTED: more than 2^31 - 1 rows in one call; per read, a
 * mismatch or deleted base 2^26 or more reference positions after start, or
 * 2^31 or more rows or read bases (field lengths of 65535 stay far inside).
 * prepare: the count / validate pass and the scan (no column memory: a cheap
 * call, also for choosing ranges by n_rows); columns: the emit pass (a lane
 * per row) and the copies into the caller's host buffers (NULL skips one).
 * Device: adam_amd/csrc/pileup.hip.  `read` = the row's read, counted from
 * r0; the Base columns hold the enum ordinal (A C T G U N X K M R Y S W B V H
 * D); slots of null entries hold 0; bitmaps are Arrow's, bits at and beyond
 * n_rows clear; countAtPosition is the constant 1. */
typedef struct bqsr_pileup_sizes {
  int64_t n_reads;
  int64_t n_rows;
  int64_t bitmap_words; /* ceil(n_rows / 64) u64 words per bitmap */
} bqsr_pileup_sizes;
typedef struct bqsr_pileup_host {
  int32_t* read;
  int64_t* position;
  int32_t* range_offset;
  int32_t* range_length;
  uint8_t* reference_base;
  uint8_t* read_base;
  int32_t* sanger_quality;
  int32_t* map_quality;
  int32_t* num_soft_clipped;
  int32_t* num_reverse_strand;
  int64_t* read_start;
  int64_t* read_end;
  uint64_t* range_valid; /* rangeOffset and rangeLength */
  uint64_t* reference_base_valid;
  uint64_t* read_base_valid;
  uint64_t* map_quality_valid;
} bqsr_pileup_host;
bqsr_status bqsr_sam_pileup_prepare(bqsr_context* ctx, bqsr_sam* s, int64_t r0, int64_t n, void* stream,
                                    bqsr_pileup_sizes* out);
bqsr_status bqsr_sam_pileup_columns(bqsr_context* ctx, bqsr_sam* s, const bqsr_pileup_host* dst, void* stream);
/* The same over a bqsr_arrow handle (the parse layout bqsr_arrow_load built).
 * mapq is not part of bqsr_arrow_chunk: it comes here, one int32 array and
 * validity bitmap (NULL: all valid; a NULL array: all null) per chunk of
 * chunk_reads[c] reads, host memory, covering the handle's reads; it is kept
 * with the handle, so later calls may pass n_chunks = 0 (never given: every
 * mapQuality null).  A null boolean reads as false (as bqsr_arrow_chunk). */
bqsr_status bqsr_arrow_pileup_prepare(bqsr_context* ctx, bqsr_arrow* a, int64_t r0, int64_t n,
                                      const int64_t* chunk_reads, const int32_t* const* mapq,
                                      const uint8_t* const* mapq_validity, int32_t n_chunks, void* stream,
                                      bqsr_pileup_sizes* out);
bqsr_status bqsr_arrow_pileup_columns(bqsr_context* ctx, bqsr_arrow* a, const bqsr_pileup_host* dst, void* stream);
/* The same emit pass with the columns LEFT ON THE DEVICE: *cols receives their
 * device addresses (n_rows entries, bitmaps ceil(n_rows / 64) words; all NULL
 * when the range has no rows) and nothing is copied to the host -- what
 * bqsr_parquet_pages_* encodes from (reads2ref -parquet_encoder device).  The
 * addresses hold until the next pileup call on the handle. */
bqsr_status bqsr_sam_pileup_device_columns(bqsr_context* ctx, bqsr_sam* s, bqsr_pileup_host* cols, void* stream);
bqsr_status bqsr_arrow_pileup_device_columns(bqsr_context* ctx, bqsr_arrow* a, bqsr_pileup_host* cols, void* stream);
/* readStart and readEnd per READ of the last prepared range, n_reads entries
 * each, into host memory: every row of read i carries read_start[i] and
 * read_end[i], so the two columns can be written as a dictionary of one entry
 * per read with the `read` column as the indices.  (A read without rows: end
 * 0, start as the parse holds it.) */
bqsr_status bqsr_sam_pileup_read_spans(bqsr_context* ctx, bqsr_sam* s, int64_t* read_start, int64_t* read_end,
                                       void* stream);
bqsr_status bqsr_arrow_pileup_read_spans(bqsr_context* ctx, bqsr_arrow* a, int64_t* read_start, int64_t* read_end,
                                         void* stream);
/* MEASUREMENT ONLY, not part of the stable interface: the device-event times
 * of the count and the emit kernel of the calling thread's last prepare /
 * columns call, in milliseconds (tools/bench_adam.py --reads2ref). */
bqsr_status bqsr_pileup_kernel_times(double* count_ms, double* emit_ms);

/* `adam mpileup` (adam-cli/.../cli/MpileupCommand.scala:37-82 over
 * PileupTraversable, adam-core/.../util/PileupTraversable.scala:83-281, with
 * MdTag.scala:38-98, 247-269 and predicates/LocusPredicate.scala): the reads of
 * a parse as pileup text, one line per (run of one referenceId, position).
 *   Reads.  LocusPredicate is applied here, to SAM / BAM input as well, on the
 *   record SAMRecordConverter produces: readMapped, primaryAlignment,
 *   !duplicateRead from the flags column as it stands (bqsr_sam_mark_duplicates
 *   changes duplicateRead), !failedVendorQualityChecks from FLAG 0x200; a
 *   FLAG-0 record has every boolean false (quirk Q2) and is dropped.  A
 *   bqsr_arrow handle carries no failedVendorQualityChecks: filter its table
 *   before the upload (adam_amd/reads2ref.py locus_filter).  The kept reads, in
 *   input order, are the job's reads; `read` in errors is the index in the
 *   handle.
 *   Events of a kept read (readToPileups).  Without CIGAR or MD: none.  Else
 *   MdTag(md, start), referencePos = start, readPos = 0, and per element
 *     M  per base a match where the MD says match (reference base = the read's
 *        base), else a mismatch where the MD has a mismatch base (reference
 *        base = the MD's, printed character = the read's base);
 *     D  per base a delete, reference base = the MD's deleted base;
 *     I  ONE insertion per element at the unchanged referencePos, no reference
 *        base, carrying the read's whole sequence;
 *     S N H P = X  nothing; both positions advance as the operator consumes
 *        (after an N the MD is looked up in the wrong place, as in reads2ref).
 *   Base is the five-value enum A C T G N: any other character in the sequence
 *   (not upper-cased) or the MD (upper-cased) throws.
 *   Segments.  A kept read whose referenceId differs from the kept read before
 *   it starts a new segment (a reference that comes back is a new segment).
 *   A line merges a position's events of one segment: matches, mismatches,
 *   deletes, insertions, each in read order.
 *   The line: name ' ' position(0-based) ' ' base-or-'?' ' ' numReads ' ', per
 *   match '.' (',' reverse strand), per mismatch the read's base (lower case
 *   on the reverse strand), per delete "-1" + the reference base, per insertion
 *   '+' + the read sequence's length + the whole sequence, '\n'.  The name is
 *   the referenceName of the position's first event.
 * Declared where the reference is loose:
 *   BQSR_ERR_UNSORTED            inside a segment a kept read's start is below
 *     the start of the kept read before it (the reference asserts only against
 *     the segment's first start, and prints positions twice otherwise);
 *     bqsr_last_error_read = the read.
 *   BQSR_ERR_REFERENCE_CONFLICT  a position's events disagree on the reference
 *     base (the reference's AssertionError); the message names the reference
 *     and the position, bqsr_last_error_read = the position.
 *   On any failure there is no text.  A read-level exception wins (the first
 *   such read in input order, that read's first exception in the reference's
 *   evaluation order), then the lowest unsorted read, then the lowest
 *   conflicting (segment, position).
 * Read-level statuses: BQSR_ERR_NULL_FIELD for a NullPointerException (a kept
 * read's null referenceId or start; a null readName, mapq -- a SAM MAPQ of 255
 * --, qual, sequence or referenceName reached by an event); BQSR_ERR_MD_PARSE
 * where MdTag.apply rejects the tag; BQSR_ERR_PILEUP for everything thrown
 * inside the CIGAR walk (a character outside A C T G N, a sequence shorter than
 * the walk, an M base the MD has as a delete or not at all, a D base without an
 * MD delete).  BQSR_ERR_UNSUPPORTED: the per-read limits of reads2ref, a start
 * below 0, more than 2^31 - 1 reads or events in one job, a key of segment,
 * position and class beyond 64 bits, or an input whose events do not fit the
 * device: one input stays resident per job (the message names the allocation).
 * prepare: everything up to every line's byte offset (walk, scan, event emit,
 * a stable radix sort by (segment, position, class), grouping); sizes out.
 * text: the largest run of whole lines from line0 within `budget` bytes,
 * formatted on the device and copied to dst (host memory, budget bytes);
 * *n_lines and *n_bytes say what was written, both 0 at line0 = n_lines.  A
 * first line longer than the budget is BQSR_ERR_INVALID_ARG, the message gives
 * its size.  Device: adam_amd/csrc/mpileup.hip. */
typedef struct bqsr_mpileup_sizes {
  int64_t n_reads;    /* reads LocusPredicate keeps */
  int64_t n_events;
  int64_t n_lines;
  int64_t text_bytes; /* of all lines */
} bqsr_mpileup_sizes;
bqsr_status bqsr_sam_mpileup_prepare(bqsr_context* ctx, bqsr_sam* s, void* stream, bqsr_mpileup_sizes* out);
bqsr_status bqsr_sam_mpileup_text(bqsr_context* ctx, bqsr_sam* s, int64_t line0, int64_t budget, char* dst,
                                  void* stream, int64_t* n_lines, int64_t* n_bytes);
/* The same over a bqsr_arrow handle loaded with MarkDuplicates' columns
 * (readName's validity and referenceId come with them; without them every
 * readName is null and referenceId is the referenceName index).  mapq as
 * bqsr_arrow_pileup_prepare takes it (kept with the handle, shared with it).
 * ref_names: the strings the handle's referenceName indices
 * (bqsr_arrow_chunk.reference) stand for.  A null boolean reads as false. */
bqsr_status bqsr_arrow_mpileup_prepare(bqsr_context* ctx, bqsr_arrow* a, const int64_t* chunk_reads,
                                       const int32_t* const* mapq, const uint8_t* const* mapq_validity,
                                       int32_t n_chunks, const char* const* ref_names, int32_t n_ref_names,
                                       void* stream, bqsr_mpileup_sizes* out);
bqsr_status bqsr_arrow_mpileup_text(bqsr_context* ctx, bqsr_arrow* a, int64_t line0, int64_t budget, char* dst,
                                    void* stream, int64_t* n_lines, int64_t* n_bytes);
/* MEASUREMENT ONLY, not part of the stable interface: device-event times, in
 * milliseconds, of the calling thread's last prepare (ms5[0] keep / compact /
 * walk, [1] event emit, [2] sort, [3] grouping) and last text call ([4] the
 * text kernel) (tools/bench_adam.py --mpileup). */
bqsr_status bqsr_mpileup_kernel_times(double* ms5);

/* Indel realignment targets: stage 1 of RealignIndels.realignIndels,
 * RealignmentTargetFinder(reads) (adam-core/.../algorithms/realignmenttarget/
 * RealignmentTargetFinder.scala:54-101 over IndelRealignmentTarget.scala:41-101,
 * 126-165, 194-231, 251-437).  One job over all reads of a handle.
 *   Rows.  reads.adamRecords2Pileup(): exactly the ADAMPileup rows of
 *   bqsr_sam_pileup_* over all reads, with the same exceptions in the same
 *   order.  No LocusPredicate, for any input: an unmapped or FLAG-0 read (quirk
 *   Q2) that has a CIGAR and an MD fails the job with BQSR_ERR_PILEUP.
 *   Rods.  Rows are grouped by position ALONE (groupBy(_.getPosition)): equal
 *   positions on two references share a rod, as in the reference.
 *   Per rod (IndelRealignmentTarget.apply).  indels: the rows with a
 *   rangeOffset (I, D and S rows: soft clips count).  matches / mismatches: the
 *   rows without one and numSoftClipped == 0, readBase == / != referenceBase.
 *   matchQuality, mismatchQuality: sums of sangerQuality as Java Ints (they
 *   wrap at 32 bits; empty: 0).  The mismatches are SNP evidence iff
 *   matchQuality == 0 || (double)mismatchQuality / (double)matchQuality >= 0.15
 *   (IEEE double; a negative ratio is below).  Every indel row gives
 *   IndelRange(indelRange, readRange): readRange = [readStart, readEnd - 1];
 *   indelRange = [position - rangeOffset, position + rangeLength - rangeOffset
 *   - 1] for a delete (readBase null), [position, position] otherwise.  Every
 *   mismatch row of a rod that keeps SNP evidence gives SNPRange(position,
 *   readRange).  Both are sets: equal tuples collapse (the rows of one
 *   multi-base insertion are one range).  A rod with both sets empty is
 *   dropped; the others are candidates, their range the hull of their
 *   elements' read ranges.
 *   The fold (joinTargets over singletons), left to right over the candidates
 *   in DECLARED order, ascending by (range start, position) -- the reference
 *   sorts by start and leaves ties to Spark, and the result depends on them.
 *   With a the last target so far and b the candidate: if
 *   TargetOrdering.overlap(a, b) -- its four clauses as written; a partial
 *   overlap is none: [1,20] then [10,30] stay two -- a = a.merge(b), else b is
 *   a new target.  merge unites the SNP sets, and sorts the united indel set
 *   and collapses runs of equal indelRange into one range with the hull of
 *   their read ranges.  A target from a single rod never went through merge
 *   and keeps two ranges with equal indelRange and different read ranges.
 *   DECLARED element order (the reference has hash sets): targets ascend by
 *   start (the fold gives that); a target's indel ranges by (indel_start,
 *   indel_end, indel_read_start, indel_read_end); its SNP ranges by (snp_site,
 *   snp_read_start, snp_read_end).
 * Read-level statuses are those of bqsr_sam_pileup_prepare (NULL_FIELD,
 * MD_PARSE, PILEUP, UNSUPPORTED): the first throwing read in input order
 * decides and bqsr_last_error_read names it.  BQSR_ERR_UNSUPPORTED also: a read
 * with rows and start < 0 (positions are sort-key bits) or 2^31 or more CIGAR
 * elements; more than 2^31 - 1 reads or rows (hence candidates or events) in a
 * job; an input that does not fit the device -- one input stays resident per
 * job, at 36 bytes of HBM per row and 80 per event beside the scan / sort
 * workspace; the message names the allocation.  On any failure there is no
 * output.  An input that yields no target is no error: zero targets.
 * prepare computes everything and keeps the results on the device; only the
 * candidates' (start, end) pairs visit the host, where the serial fold runs.
 * fetch copies the columns asked for (a NULL pointer skips one): per target
 * start and end; indel_offset / snp_offset with n_targets + 1 entries each
 * (always at least the one 0); n_indels indel and n_snps SNP ranges.  Device:
 * adam_amd/csrc/realign_targets.hip. */
typedef struct bqsr_realign_targets_sizes {
  int64_t n_reads;
  int64_t n_rows;       /* ADAMPileup rows */
  int64_t n_candidates; /* rods with evidence */
  int64_t n_targets;
  int64_t n_indels;     /* indel ranges of all targets */
  int64_t n_snps;       /* SNP ranges of all targets */
} bqsr_realign_targets_sizes;
typedef struct bqsr_realign_targets_host {
  int64_t* target_start;
  int64_t* target_end;
  int64_t* indel_offset;
  int64_t* snp_offset;
  int64_t* indel_start;
  int64_t* indel_end;
  int64_t* indel_read_start;
  int64_t* indel_read_end;
  int64_t* snp_site;
  int64_t* snp_read_start;
  int64_t* snp_read_end;
} bqsr_realign_targets_host;
bqsr_status bqsr_sam_realign_targets_prepare(bqsr_context* ctx, bqsr_sam* s, void* stream,
                                             bqsr_realign_targets_sizes* out);
bqsr_status bqsr_sam_realign_targets_fetch(bqsr_context* ctx, bqsr_sam* s, const bqsr_realign_targets_host* dst,
                                           void* stream);
/* The same over a bqsr_arrow handle; mapq is no part of a target and is not
 * needed.  A null boolean reads as false. */
bqsr_status bqsr_arrow_realign_targets_prepare(bqsr_context* ctx, bqsr_arrow* a, void* stream,
                                               bqsr_realign_targets_sizes* out);
bqsr_status bqsr_arrow_realign_targets_fetch(bqsr_context* ctx, bqsr_arrow* a, const bqsr_realign_targets_host* dst,
                                             void* stream);
/* MEASUREMENT ONLY, not part of the stable interface: times, in milliseconds,
 * of the calling thread's last prepare: by device events ms7[0] the count
 * kernel, [1] row scan and emit, [2] the row sort, [3] rods and events, [4]
 * candidates (hulls and their sort), [6] the targets' sets; by the host clock
 * [5] the fold (tools/bench_adam.py --realign-targets). */
bqsr_status bqsr_realign_targets_kernel_times(double* ms7);

/* `adam aggregate_pileups` and what `reads2ref -aggregate` would compute
 * (adam-cli/.../cli/PileupAggregator.scala:27-57 over PileupAggregator.
 * aggregate, adam-core/.../rdd/PileupAggregator.scala:25-219): ADAMPileup rows
 * grouped by (referenceId, position) and, within a position, by (readBase,
 * rangeOffset, recordGroupSample); every group folded into one row.  Each of
 * the three inner components is nullable and null is a value of its own (a null
 * rangeOffset is not 0, a null sample is not "").
 * The reference leaves two orders to Spark's shuffle and to a hash map; this
 * interface DECLARES them:
 *   fold order    rows fold in input row order: the order of the add calls,
 *                 then the row order within an add.
 *   output order  groups ascend by (referenceId, position, readBase ordinal,
 *                 rangeOffset, sample code), integers signed, nulls first in
 *                 every component.  The caller gives samples as int32 codes;
 *                 codes that rank the distinct sample strings in byte order
 *                 make this the byte order of the strings.
 * A group of one row passes through, except mapQuality = mapQuality /
 * countAtPosition and sangerQuality = sangerQuality / countAtPosition (so
 * aggregating an aggregated file divides again, as in the reference).  A group
 * of n >= 2 rows is the reference's reduce, a left fold whose accumulator is a
 * built record: C = c_1, M = m_1, S = s_1, then for k = 2..n
 *   M = M * C + m_k * c_k;  S = S * C + s_k * c_k;  C = C + c_k
 * (M and S use the old C: the accumulator's quality is multiplied by its
 * accumulated count -- the reference's quirk, order-dependent and factorial in
 * depth), all in Java int arithmetic, wrapping mod 2^32; at the end mapQuality
 * = M / C, sangerQuality = S / C, countAtPosition = C, the division truncating
 * toward zero and Int.MinValue / -1 = Int.MinValue.  numSoftClipped and
 * numReverseStrand are wrapping int sums, readStart the min, readEnd the max;
 * referenceId, position, rangeOffset, rangeLength, referenceBase and readBase
 * are the group's first row's.  The string columns are the caller's: fetch
 * returns every group's rows in fold order (offsets into order) for them.
 * Errors (bqsr_last_error_read = the row, counted over all adds; no result).
 * The reference groups every row before it folds any, and so does the order
 * declared here: first what throws while grouping, then what the folds throw,
 * and within either the LOWEST offending input row decides (on one row
 * NULL_FIELD before PILEUP).
 *   grouping  BQSR_ERR_NULL_FIELD  a null referenceId or position
 *             (ReferencePosition.apply unboxes them)
 *             BQSR_ERR_UNSUPPORTED a sample code outside [0, 2^22 - 2] (and,
 *             from the add calls, more than 2^31 - 1 rows in one handle)
 *   folds     BQSR_ERR_NULL_FIELD  in any row a null mapQuality, sangerQuality
 *             or countAtPosition; in a row of a group of two or more a null
 *             numSoftClipped, numReverseStrand, readStart or readEnd (a lone
 *             row with those nulls passes through)
 *             BQSR_ERR_PILEUP      a group whose C is 0 (Java's
 *             ArithmeticException), reported at the group's first row
 * The handle keeps every added row on the device (about 70 bytes a row; run
 * needs some 30 bytes a row more, plus the sort's scratch, while it runs).
 * add_host: n_rows rows from host columns.  A NULL value column is a column of
 *   nulls (rg_code is required); a *_valid pointer is an Arrow validity bitmap
 *   of the add's rows (ceil(n_rows / 8) bytes, NULL: all valid).  Base columns
 *   hold the enum ordinal.  rg_code: any int32 that is equal for rows whose ten
 *   recordGroup* fields are equal; it only feeds uniform_rg.  name_code: the
 *   caller's code of the row's readName, handed back by fetch (NULL: the
 *   row's index in the handle).
 * bqsr_sam_pileup_agg_add / bqsr_arrow_pileup_agg_add: the rows of the last
 *   *_pileup_prepare on that parse, written by the emit pass straight into the
 *   handle's columns (no host copy).  sample_code and rg_code: host arrays, one
 *   entry per read of the prepared range (a negative sample code: null sample).
 *   referenceId is the parse's (SAM / BAM: the @SQ index, null for "*"; a
 *   bqsr_arrow handle: its referenceId column, loaded as for MarkDuplicates, a
 *   negative one reading as null); countAtPosition is 1; a row's name code is
 *   name_base + its read's index in the prepared range (the caller's ordinal
 *   of the read; below 2^31).
 * run: keys, sort, heads, the two scans, emit (adam_amd/csrc/pileup_agg.hip).
 *   Adding rows afterwards discards the result; run may be called again.
 * fetch: the result of the last successful run into host buffers (NULL skips
 *   one): the group columns [n_groups]; validity words [bitmap_words] (bits at
 *   and beyond n_groups clear; slots of null entries hold 0; the columns
 *   without a word are never null); first_row = the group's first input row;
 *   offsets [n_groups + 1] into order [n_rows], the input rows sorted by group,
 *   a group's rows in fold order; names [n_rows]: the name codes of the rows of
 *   order; uniform_rg: bit set where every row of the
 *   group has one rg_code. */
typedef struct bqsr_pileup_agg bqsr_pileup_agg;
typedef struct bqsr_pileup_agg_rows {
  int64_t n_rows;
  const int32_t* reference_id;
  const int64_t* position;
  const int32_t* range_offset;
  const int32_t* range_length;
  const uint8_t* reference_base;
  const uint8_t* read_base;
  const int32_t* sanger_quality;
  const int32_t* map_quality;
  const int32_t* num_soft_clipped;
  const int32_t* num_reverse_strand;
  const int32_t* count_at_position;
  const int64_t* read_start;
  const int64_t* read_end;
  const int32_t* sample_code;
  const int32_t* rg_code;
  const int32_t* name_code;
  const uint8_t* reference_id_valid;
  const uint8_t* position_valid;
  const uint8_t* range_offset_valid;
  const uint8_t* range_length_valid;
  const uint8_t* reference_base_valid;
  const uint8_t* read_base_valid;
  const uint8_t* sanger_quality_valid;
  const uint8_t* map_quality_valid;
  const uint8_t* num_soft_clipped_valid;
  const uint8_t* num_reverse_strand_valid;
  const uint8_t* count_at_position_valid;
  const uint8_t* read_start_valid;
  const uint8_t* read_end_valid;
  const uint8_t* sample_code_valid;
} bqsr_pileup_agg_rows;
typedef struct bqsr_pileup_agg_sizes {
  int64_t n_rows;
  int64_t n_groups;
  int64_t bitmap_words; /* ceil(n_groups / 64) u64 words per bitmap */
} bqsr_pileup_agg_sizes;
typedef struct bqsr_pileup_agg_host {
  int32_t* reference_id;
  int64_t* position;
  int32_t* range_offset;
  int32_t* range_length;
  uint8_t* reference_base;
  uint8_t* read_base;
  int32_t* sanger_quality;
  int32_t* map_quality;
  int32_t* num_soft_clipped;
  int32_t* num_reverse_strand;
  int32_t* count_at_position;
  int64_t* read_start;
  int64_t* read_end;
  uint32_t* first_row;
  uint32_t* offsets;
  uint32_t* order;
  int32_t* names;
  uint64_t* range_offset_valid;
  uint64_t* range_length_valid;
  uint64_t* reference_base_valid;
  uint64_t* read_base_valid;
  uint64_t* num_soft_clipped_valid;
  uint64_t* num_reverse_strand_valid;
  uint64_t* read_start_valid;
  uint64_t* read_end_valid;
  uint64_t* uniform_rg;
} bqsr_pileup_agg_host;
bqsr_status bqsr_pileup_agg_create(bqsr_context* ctx, bqsr_pileup_agg** out);
void bqsr_pileup_agg_destroy(bqsr_pileup_agg* agg);
bqsr_status bqsr_pileup_agg_add_host(bqsr_pileup_agg* agg, const bqsr_pileup_agg_rows* rows, void* stream);
bqsr_status bqsr_sam_pileup_agg_add(bqsr_context* ctx, bqsr_sam* s, bqsr_pileup_agg* agg, const int32_t* sample_code,
                                    const int32_t* rg_code, int64_t name_base, void* stream);
bqsr_status bqsr_arrow_pileup_agg_add(bqsr_context* ctx, bqsr_arrow* a, bqsr_pileup_agg* agg,
                                      const int32_t* sample_code, const int32_t* rg_code, int64_t name_base,
                                      void* stream);
bqsr_status bqsr_pileup_agg_run(bqsr_pileup_agg* agg, void* stream, bqsr_pileup_agg_sizes* out);
bqsr_status bqsr_pileup_agg_fetch(bqsr_pileup_agg* agg, const bqsr_pileup_agg_host* dst, void* stream);
/* MEASUREMENT ONLY, not part of the stable interface: device-event times of
 * the calling thread's last run, in ms: the keys kernel; the sort (key
 * gathers and radix passes, and the host's look at the error word before
 * them); heads and the two scans; emit (tools/bench_adam.py --aggregate). */
bqsr_status bqsr_pileup_agg_kernel_times(double* keys_ms, double* sort_ms, double* scans_ms, double* emit_ms);

/* MarkDuplicates across the partitions of one input (the reference's
 * groupBy spans every partition of the RDD, MarkDuplicates.scala:43-58).
 * add: one partition's parse (partitions in input order, each parsed with
 * the same header); its reads get global indices after those added before.
 * Per read the set keeps a compact record on the device (two 64-bit hashes
 * of (rg, QNAME), class, packed 5' position, score, library rank; 31 bytes),
 * so partitions need not stay resident.  finish: buckets, groups and the
 * duplicate bit of every read (the passes of bqsr_sam_mark_duplicates);
 * records are released.  apply: a parse of partition `part` (the same text
 * as added) gets its reads' duplicateRead bits, as bqsr_sam_mark_duplicates
 * leaves them.  Reads of different partitions share a bucket when both
 * hashes agree (names are not compared across partitions: a 128-bit
 * collision would merge two buckets).  BQSR_ERR_UNSUPPORTED for more than
 * 2^32 - 1 reads or positions / libraries beyond the packed keys;
 * BQSR_ERR_INVALID_ARG for partitions whose headers name other libraries.
 * The packed keys' limits are bqsr_sam_mark_duplicates': 32767 contigs
 * (referenceId 0..32766) and 4095 distinct LB values.  There is no host form
 * here: when any read added is a primary mapped read on a later contig, or
 * carries a library of rank 4096 or more, bqsr_dup_set_finish fails with
 * BQSR_ERR_UNSUPPORTED and no read is marked. */
typedef struct bqsr_dup_set bqsr_dup_set;
bqsr_status bqsr_dup_set_create(bqsr_context* ctx, int64_t reads_hint, bqsr_dup_set** out);
bqsr_status bqsr_dup_set_add(bqsr_dup_set* d, const bqsr_sam* s);
bqsr_status bqsr_dup_set_finish(bqsr_dup_set* d, int64_t* n_duplicates);
bqsr_status bqsr_dup_set_apply(bqsr_dup_set* d, int64_t part, bqsr_sam* s, int64_t* n_duplicates);
void bqsr_dup_set_destroy(bqsr_dup_set* d);

/* `adam compare` and `adam findreads` (adam-cli/.../cli/CompareAdam.scala,
 * FindReads.scala over rdd/comparisons/ComparisonTraversalEngine.scala:40-59
 * and metrics/AvailableComparisons.scala:44-177): the reads of two inputs in
 * ReadBuckets by (recordGroupId, readName), the buckets joined by readName
 * (two buckets of one name in different record groups both join), and the
 * five comparisons -- 0 overmatched, 1 dupemismatch, 2 positions, 3 mapqs,
 * 4 baseqs, DefaultComparisons' order -- aggregated into histograms with
 * 64-bit counts.  Both inputs are resident at once, one parse per side.
 *
 * options (NULL: the defaults): hash_bits masks both the bucket hash and the
 * name hash of the join down to that many bits (0 or 64: unmasked; smaller
 * values are for tests, which make collisions common with them);
 * utf8_1 / utf8_2: the side's QUAL bytes are UTF-8 and one Java char each (a
 * 4-byte sequence two), else one char per byte; comparisons: bit k selects
 * comparison k; flush_chars: the chars a workgroup of the baseqs pass takes
 * between two flushes of its private 32-bit table (0: 2^31; at least 16384,
 * at most BQSR_COMPARE_MAX_FLUSH_CHARS; tests lower it); baseq_groups: the
 * workgroups of the baseqs pass (0: two per compute unit; tests lower it so
 * that a workgroup takes several chunks and flushes in between).
 *
 * bqsr_compare_sam runs the selected comparisons and those the filter terms
 * name.  A term is (comparison, op, a, b): op 0 `=`, 1 `!=`, 2 `<`, 3 `>`;
 * overmatched takes `=` with a = 0 / 1, positions `=`, `<`, `>` with a,
 * the point comparisons `=`, `!=` with the 32-bit point (a, b)
 * (bqsr_compare_check_terms: BQSR_ERR_INVALID_ARG otherwise, no device
 * call).  A joined pair is a row when every term is met by some value its
 * comparison produced for the pair; rows are ordered by bucket 1's first
 * read, then bucket 2's.
 *
 * Results: the totals, uniques and the two small histograms in `out`;
 * positions and mapqs as (value, count) lists (bqsr_compare_values: int64
 * values for positions, (uint32 mapq1 << 32 | uint32 mapq2) for mapqs, counts
 * int64, n_positions / n_mapqs entries, ascending); baseqs as a 256 x 256
 * table of int64 indexed by the two scores' low bytes (bqsr_compare_baseqs);
 * the rows as the two buckets' allReads.head read indices (bqsr_compare_rows,
 * n_rows entries each).  They stay with the handle until its next run.
 *
 * out->collision = 1 (status BQSR_OK, nothing else filled in): two
 * (recordGroupId, readName) keys of one input share a hash -- detected by
 * comparing every read's name with its run head's; the caller takes another
 * path.  A collision of name hashes in the join is harmless: candidates are
 * accepted by their bytes.
 * BQSR_ERR_NULL_FIELD where the reference unboxes a null -- start of a
 * singly matched read whose referenceIds compare equal (positions), mapq
 * (mapqs), qual (baseqs): the first comparison in order that met one, side 1
 * before side 2, the first such read of that side (out->null_comparison,
 * null_side, null_read; bqsr_last_error_read).  A comparison neither selected
 * nor named by a term never fails the call.
 * BQSR_ERR_SAM_PARSE for QUAL bytes of a UTF-8 side that are no UTF-8.
 * BQSR_ERR_UNSUPPORTED: more than BQSR_COMPARE_MAX_READS reads on a side,
 * joined pairs, or matched read pairs; more than 16 terms. */
#define BQSR_COMPARE_MAX_READS 4294967295ll
#define BQSR_COMPARE_MAX_FLUSH_CHARS 2147483648ll
typedef struct bqsr_compare bqsr_compare;
typedef struct bqsr_compare_options {
  int32_t hash_bits;
  int32_t utf8_1, utf8_2;
  uint32_t comparisons;
  int64_t flush_chars;
  int32_t baseq_groups;
  int32_t reserved; /* 0 */
} bqsr_compare_options;
typedef struct bqsr_compare_term {
  int32_t comparison, op;
  int64_t a, b;
} bqsr_compare_term;
typedef struct bqsr_compare_result {
  int64_t total1, unique1, total2, unique2; /* buckets, not reads */
  int64_t n_pairs;                          /* joined pairs */
  int64_t overmatched[2];                   /* false, true */
  int64_t dupemismatch[4];                  /* (d1, d2) at 2 * d1 + d2 */
  int64_t n_positions, n_mapqs, n_rows;
  int32_t collision;
  int32_t null_comparison, null_side; /* NULL_FIELD: the comparison, side 1 or 2 */
  int32_t flushes;                    /* flushes of private tables in the baseqs pass */
  int64_t null_read;
  int64_t baseq_chars; /* chars the baseqs pass zipped */
} bqsr_compare_result;
bqsr_status bqsr_compare_create(bqsr_context* ctx, const bqsr_compare_options* options, bqsr_compare** out);
void bqsr_compare_destroy(bqsr_compare* c);
bqsr_status bqsr_compare_check_terms(const bqsr_compare_term* terms, int32_t n_terms);
bqsr_status bqsr_compare_sam(bqsr_compare* c, const bqsr_sam* s1, const bqsr_sam* s2, const bqsr_compare_term* terms,
                             int32_t n_terms, void* stream, bqsr_compare_result* out);
/* The same over sides of either kind: exactly one of `sam` (a bqsr_sam_parse
 * / bqsr_bam_parse result) and `arrow` (a bqsr_arrow_load result with the
 * read_name and reference_id columns of its chunks given) is set.  For an
 * Arrow side, firstOfPair and mapq are not part of bqsr_arrow_chunk: they
 * come here, per chunk of chunk_reads[k] reads covering the load's reads, as
 * host buffers at array offset 0 -- first_of_pair[k] a boolean bitmap and
 * mapq[k] an int32 array, each with a validity bitmap (a NULL validity: all
 * valid; a NULL array or list: all null).  They are read before the call
 * returns.  A null boolean reads as false; a null readName is one name of its
 * own, distinct from ""; referenceId, start, mapq and qual may be null (see
 * BQSR_ERR_NULL_FIELD above); qual chars are the load's (UTF-8 -> Java chars),
 * so utf8_1 / utf8_2 do not apply to an Arrow side. */
typedef struct bqsr_compare_side {
  const bqsr_sam* sam;
  const bqsr_arrow* arrow;
  const int64_t* chunk_reads;
  const uint8_t* const* first_of_pair;
  const uint8_t* const* first_of_pair_validity;
  const int32_t* const* mapq;
  const uint8_t* const* mapq_validity;
  int32_t n_chunks;
} bqsr_compare_side;
bqsr_status bqsr_compare_sides(bqsr_compare* c, const bqsr_compare_side* side1, const bqsr_compare_side* side2,
                               const bqsr_compare_term* terms, int32_t n_terms, void* stream,
                               bqsr_compare_result* out);
bqsr_status bqsr_compare_values(const bqsr_compare* c, int32_t comparison, void* values, int64_t* counts);
bqsr_status bqsr_compare_baseqs(const bqsr_compare* c, int64_t* table);
bqsr_status bqsr_compare_rows(const bqsr_compare* c, uint32_t* head1, uint32_t* head2);
/* MEASUREMENT ONLY: the device-event times of the handle's last run: the
 * join, the scalar pass and the baseqs pass (with the UTF-8 decode pass of a
 * side read as UTF-8), in milliseconds (tools/bench_compare.py). */
bqsr_status bqsr_compare_kernel_times(const bqsr_compare* c, double* join_ms, double* scalar_ms, double* baseqs_ms);

/* adamSave's GZIP part files (AdamRDDFunctions.scala:37-48 through
 * parquet-mr; ParquetArgs.scala:27: GZIP by default).  `in` is a Parquet file
 * written UNCOMPRESSED (Arrow's writer: schema, encodings, dictionary pages,
 * statistics), here rewritten to `path` with every page a gzip member:
 * the columns named in `huffman_cols` (comma-separated top-level names, e.g.
 * "qual,sequence") as one dynamic-Huffman DEFLATE block of literals, the
 * others by libdeflate (zlib when absent) at `level` (zlib's default 6 is
 * Hadoop's GzipCodec); page headers, column-chunk metadata and the footer
 * re-encoded with the new sizes and offsets.  Data page v1 and dictionary
 * pages; no page index, bloom filter or external column chunks
 * (BQSR_ERR_INVALID_ARG otherwise).  `threads` compress pages in parallel.
 * *out_len: bytes written. */
bqsr_status bqsr_parquet_gzip(const uint8_t* in, int64_t in_len, const char* path, int32_t level,
                              const char* huffman_cols, int32_t threads, int64_t* out_len);
/* One gzip member of n bytes into out (cap bytes; *out_len the size, also
 * when it does not fit): huffman != 0 the literal-only Huffman block, else
 * libdeflate / zlib at `level` (tests). */
bqsr_status bqsr_gzip_bytes(const uint8_t* in, int64_t n, int32_t huffman, int32_t level, uint8_t* out, int64_t cap,
                            int64_t* out_len);

/* Parquet data page bodies built on the device (adam_amd/csrc/
 * parquet_pages.hip): one column chunk at a time, from columns in DEVICE
 * memory, cut into V1 data pages of page_rows rows (a multiple of 64; the
 * last page may be short).  The caller adds page headers, dictionary pages,
 * the codec and the footer (adam_amd/parquet_pages.py).  A column is
 * described by a bqsr_parquet_column; row g of it is
 *   null    when `validity` (an Arrow bitmap in u64 words) is given and bit g
 *           is clear; else with i = gather ? gather[g] : g, when i is outside
 *           [0, src_n); else with v = src[i] (src_width 1: uint8, 4: int32,
 *           8: int64) and a `remap` table, when v is outside [0, remap_n) or
 *           remap[v] < 0;
 *   else    (remap ? remap[v] : v) - base.
 * A page body is, in order:
 *   definition levels (max level 1, RLE encoding): u32 LE length, then ONE
 *     bit-packed run of the hybrid encoding -- varint(ceil(rows / 8) << 1 | 1)
 *     and the page's ceil(rows / 8) bitmap bytes (bit set = value present,
 *     padding bits clear);
 *   BQSR_PARQUET_PLAIN_INT32 / _INT64: the page's non-null values in row
 *     order, 4 / 8 bytes LE each;
 *   BQSR_PARQUET_DICT_INDEX: one byte bit_width (w, 1..32), then the page's
 *     non-null values (their low w bits) in row order under this BLOCK RULE:
 *     the values are taken in blocks of 64; a full block whose 64 values are
 *     equal is one RLE run, varint(64 << 1) = 80 01 and the value in
 *     ceil(w / 8) bytes LE; any other block is one bit-packed run,
 *     varint(groups << 1 | 1) with groups = ceil(values / 8), then groups * w
 *     bytes, values LSB first, the last group zero-padded to 8 values.
 *     Adjacent equal runs are not merged: the bytes are a pure function of
 *     the column.
 *   BQSR_PARQUET_PLAIN_BYTE_ARRAY (bqsr_parquet_pages_size_strings: an Arrow
 *     string column -- int32 offsets [n_rows + 1], bytes, an optional validity
 *     bitmap in u64 words): for every non-null row of the page, in row order,
 *     a u32 LE length and the bytes offsets[r] .. offsets[r + 1].  A null row
 *     gives nothing, whatever its offsets span.
 *   BQSR_PARQUET_PLAIN_BOOLEAN (bqsr_parquet_pages_size_bools: an Arrow bitmap
 *     of values in u64 words, bit r = row r, and an optional validity bitmap):
 *     the page's non-null values one bit each, LSB first, in
 *     ceil(non_nulls / 8) bytes, the last byte's padding bits clear.  Bits of
 *     either bitmap beyond n_rows are not read into the output.
 * The last two kinds have size calls of their own (no bqsr_parquet_column
 * describes them); the emit call after any size call writes the kind that
 * call left in the handle, and the column's buffers must stay as they are
 * until then.
 * size: the passes up to the chunk's exact size (nothing is allocated for the
 * output before it is known); emit: the write pass and ONE copy of the bodies
 * and one of the page table into host memory (bodies: body_bytes bytes, pages:
 * n_pages entries; offsets are into `bodies`).  One emit per size call.
 * minmax: the least and greatest non-null value and their count (min > max
 * when there is none): a caller's dense-range dictionary [min, max] with base
 * = min.  An encoder handle keeps its device scratch across calls and serves
 * one thread at a time.  BQSR_ERR_INVALID_ARG: a kind, width or page_rows
 * outside the above, remap or base on a PLAIN column, more than 2^31 - 1 rows,
 * a null source (offsets, bytes, bits) with rows, an emit without a size call. */
enum {
  BQSR_PARQUET_PLAIN_INT32 = 0,
  BQSR_PARQUET_PLAIN_INT64 = 1,
  BQSR_PARQUET_DICT_INDEX = 2,
  BQSR_PARQUET_PLAIN_BYTE_ARRAY = 3,
  BQSR_PARQUET_PLAIN_BOOLEAN = 4
};
typedef struct bqsr_parquet_pages bqsr_parquet_pages;
typedef struct bqsr_parquet_column {
  int32_t kind;
  int32_t src_width;
  const void* src;
  int64_t src_n; /* elements of src */
  const int32_t* gather;
  const int32_t* remap;
  int32_t remap_n;
  int32_t bit_width;
  int64_t base;
  const uint64_t* validity;
} bqsr_parquet_column;
typedef struct bqsr_parquet_page {
  int64_t offset; /* of the body in the chunk's bodies */
  int64_t bytes;
  int64_t rows;
  int64_t non_nulls;
} bqsr_parquet_page;
typedef struct bqsr_parquet_pages_sizes {
  int64_t n_pages;
  int64_t body_bytes;
} bqsr_parquet_pages_sizes;
bqsr_status bqsr_parquet_pages_create(bqsr_context* ctx, bqsr_parquet_pages** out);
void bqsr_parquet_pages_destroy(bqsr_parquet_pages* enc);
bqsr_status bqsr_parquet_pages_size(bqsr_parquet_pages* enc, const bqsr_parquet_column* col, int64_t n_rows,
                                    int64_t page_rows, void* stream, bqsr_parquet_pages_sizes* out);
bqsr_status bqsr_parquet_pages_size_strings(bqsr_parquet_pages* enc, const int32_t* offsets, const uint8_t* bytes,
                                            const uint64_t* validity, int64_t n_rows, int64_t page_rows, void* stream,
                                            bqsr_parquet_pages_sizes* sizes);
bqsr_status bqsr_parquet_pages_size_bools(bqsr_parquet_pages* enc, const uint64_t* bits, const uint64_t* validity,
                                          int64_t n_rows, int64_t page_rows, void* stream,
                                          bqsr_parquet_pages_sizes* sizes);
bqsr_status bqsr_parquet_pages_emit(bqsr_parquet_pages* enc, uint8_t* bodies, bqsr_parquet_page* pages, void* stream);
bqsr_status bqsr_parquet_pages_minmax(bqsr_parquet_pages* enc, const bqsr_parquet_column* col, int64_t n_rows,
                                      void* stream, int64_t* min_out, int64_t* max_out, int64_t* non_nulls);
/* MEASUREMENT ONLY: the device-event times of the calling thread's last size
 * call (levels, compaction, item sizes and the two scans) and of the emit call
 * after it, in milliseconds (tools/bench_adam.py --reads2ref). */
bqsr_status bqsr_parquet_pages_kernel_times(double* size_ms, double* emit_ms);

/* Page bodies compressed with snappy on the device (adam_amd/csrc/
 * snappy_pages.hip).  `in` (host memory) holds n_pages pages laid end to end:
 * page i is in[page_off[i], page_off[i + 1]) (any byte offsets, not
 * decreasing; a page is below 2^31 bytes).  The bytes are uploaded, every page
 * compressed, the pages packed on the device and only the packed bytes come
 * back: page i is out[out_off[i], out_off[i + 1]).  out_off[n_pages] is the
 * total, also when it exceeds cap (BQSR_ERR_INVALID_ARG then, nothing
 * written); 32 + n + n / 6 bytes per page of n bytes always suffice.
 * THE FORMAT (raw snappy, a pure function of the page's bytes: no level, no
 * dependence on timing).  A compressed page is varint(n) followed by the
 * elements of its ceil(n / 65536) blocks in order (the last block may be
 * short; n == 0 gives the single byte 00).  Every block is compressed on its
 * own, and within a block:
 *   - no copy reaches before the block's first byte;
 *   - a copy has length 4..64 and offset 1..65535;
 *   - a copy is written in the 1-byte-offset form (tag 01) when its length is
 *     4..11 and its offset is below 2048, otherwise in the 2-byte-offset form
 *     (tag 10); the 4-byte-offset form never appears;
 *   - the positions the parse leaves as literals are merged into maximal runs
 *     within the block, each run one literal element: the length inline for
 *     runs up to 60, in one extra byte up to 256, in two up to 65536.
 * The parse is greedy over three match candidates per position (distance 1,
 * the first position of the position's hash bucket in its chunk of 2048, the
 * bucket's highest position of the earlier chunks), the longest winning, the
 * nearer one on a tie; a match is extended to at most 64 bytes. */
bqsr_status bqsr_snappy_pages(bqsr_context* ctx, const uint8_t* in, const int64_t* page_off, int64_t n_pages,
                              void* stream, uint8_t* out, int64_t cap, int64_t* out_off);
/* The same block routine compiled for the host, a lane at a time: the bytes
 * bqsr_snappy_pages gives, without a context, a stream or a device call.  For
 * tests on a machine without a GPU; far slower than a host snappy. */
bqsr_status bqsr_snappy_pages_host(const uint8_t* in, const int64_t* page_off, int64_t n_pages, uint8_t* out,
                                   int64_t cap, int64_t* out_off);
/* The encoder's pages compressed before they come down.  compress: in place
 * of bqsr_parquet_pages_emit after a size call -- the write pass, the bodies
 * kept on the device, every page compressed as bqsr_snappy_pages does it, the
 * packed size into *comp_bytes.  codec: BQSR_PARQUET_CODEC_SNAPPY (any other
 * value: BQSR_ERR_INVALID_ARG).  fetch: ONE copy of the packed pages into comp
 * (comp_bytes bytes) and the two tables: pages (n_pages entries; offset and
 * bytes are those of the RAW body, which the page header needs) and comp_off
 * [n_pages + 1], page i's compressed bytes being comp[comp_off[i],
 * comp_off[i + 1]).  One compress and one fetch per size call.
 * BQSR_ERR_INVALID_ARG: a compress without a size call, a fetch without a
 * compress, an emit after a compress. */
enum { BQSR_PARQUET_CODEC_SNAPPY = 1 };
bqsr_status bqsr_parquet_pages_compress(bqsr_parquet_pages* enc, int32_t codec, void* stream, int64_t* comp_bytes);
bqsr_status bqsr_parquet_pages_fetch(bqsr_parquet_pages* enc, uint8_t* comp, bqsr_parquet_page* pages,
                                     int64_t* comp_off, void* stream);
/* MEASUREMENT ONLY: the device-event times of the calling thread's last
 * bqsr_parquet_pages_compress or bqsr_snappy_pages: the block kernel and the
 * pack kernel, in milliseconds (tools/bench_adam.py --parquet-encoder). */
bqsr_status bqsr_parquet_pages_compress_times(double* snappy_ms, double* pack_ms);

/* adam2sam: ADAMRecord Parquet out as SAM or BAM.  The records of an Arrow
 * table are rendered as SAM lines on the device (adam_lines.hip) and the text
 * parsed like SAM input, so the result is an ordinary bqsr_sam: the SAM text
 * sink, the BAM encoder, both compressors, the BAM index, bqsr_sam_sort and
 * bqsr_sam_flagstat take it as they take a bqsr_sam_parse / bqsr_bam_parse
 * result.  One bqsr_adam_lines_chunk per Arrow record batch, its buffers as
 * they are (array offsets 0; strings as bqsr_arrow_strings; a NULL column is
 * all null; a NULL validity: all valid; a null boolean reads as false).
 * reference / mate_reference: int32 indices of referenceName / mateReference
 * into the reference names (ref_names_blob cut by ref_name_offsets [n_ref +
 * 1]).  `header`: the header lines of the text (nothing else; "" allowed) --
 * RNAME becomes a referenceName, and BAM's refID, only through its @SQ lines.
 *
 * A record's line is the inverse of SAMRecordConverter.convert
 * (core/converters/SAMRecordConverter.scala:26-144), fields in SAM's order:
 *   QNAME CIGAR SEQ QUAL  the column's bytes (readName, cigar, sequence,
 *            qual); null or empty: "*".  Bytes are copied as they are (the
 *            caller re-encodes a qual chunk with chars above 0x7F: one byte
 *            c & 0xFF per Java char, as parquet.py reads qual);
 *   FLAG     0 when all eleven booleans are false (the converter reads FLAG 0
 *            that way, and FLAG 0x104 too, which therefore comes back as 0);
 *            else 0x1 readPaired, 0x2 properPair, 0x4 !readMapped, 0x8
 *            readPaired && !mateMapped, 0x10 readNegativeStrand, 0x20
 *            mateNegativeStrand, 0x40 firstOfPair, 0x80 secondOfPair, 0x100
 *            !primaryAlignment, 0x200 failedVendorQualityChecks, 0x400
 *            duplicateRead;
 *   RNAME    the reference name, "*" when null;
 *   POS      start + 1, 0 when null;
 *   MAPQ     mapq; when null 255 with a referenceName (the one case in which
 *            the converter drops a MAPQ), else 0;
 *   RNEXT    "*" when null, "=" for RNAME's index, else the name;
 *   PNEXT    mateAlignmentStart + 1, 0 when null;
 *   TLEN     0 (ADAMRecord has no field for it);
 *   optional fields  `attributes` cut at its TABs, the fields in reverse (the
 *            converter prepends: htsjdk's order again), then MD:Z:<
 *            mismatchingPositions> when that is not null.  Null or empty
 *            attributes give none.  No RG tag is made from recordGroupName:
 *            it is among the attributes already.
 * Refused, naming the first such record (bqsr_last_error_read), nothing
 * produced -- BQSR_ERR_UNSUPPORTED, a record SAM cannot hold (as the BAM
 * encoder's refusals): TAB, LF or CR inside readName, cigar, sequence, qual
 * or mismatchingPositions; LF or CR inside attributes; start or
 * mateAlignmentStart outside [0, 2^31 - 2]; mapq outside [0, 255] --
 * BQSR_ERR_SAM_PARSE, a malformed record (as bqsr_bam_parse's): an attribute
 * that is not [A-Za-z][A-Za-z0-9]:[AifZHB]:..., a reference index outside
 * [0, n_ref).  A record with both is reported as malformed.  The whole
 * table's buffers and its text stay on the device for the call:
 * BQSR_ERR_UNSUPPORTED when the text does not fit. */
typedef struct bqsr_adam_lines_chunk {
  int64_t n_reads;
  bqsr_arrow_strings read_name, cigar, sequence, qual, attributes, md; /* md = mismatchingPositions */
  const int64_t* start;
  const uint8_t* start_validity;
  const int64_t* mate_start; /* mateAlignmentStart */
  const uint8_t* mate_start_validity;
  const int32_t* mapq;
  const uint8_t* mapq_validity;
  const int32_t* reference;
  const uint8_t* reference_validity;
  const int32_t* mate_reference;
  const uint8_t* mate_reference_validity;
  /* readPaired, properPair, readMapped, mateMapped, readNegativeStrand, mateNegativeStrand, firstOfPair,
   * secondOfPair, primaryAlignment, failedVendorQualityChecks, duplicateRead */
  const uint8_t* bools[11];
  const uint8_t* bools_validity[11];
} bqsr_adam_lines_chunk;
bqsr_status bqsr_arrow_sam_lines(bqsr_context* ctx, const bqsr_adam_lines_chunk* chunks, int32_t n_chunks,
                                 const uint8_t* ref_names_blob, const int64_t* ref_name_offsets, int32_t n_ref,
                                 const char* header, int64_t header_bytes, void* stream, bqsr_sam** out);
/* MEASUREMENT ONLY: this thread's last bqsr_arrow_sam_lines: the uploads, the
 * length pass and the write pass by device events, the parse of the text by
 * the host's clock, in milliseconds (tools/bench_adam.py). */
bqsr_status bqsr_adam_lines_kernel_times(double* upload_ms, double* len_ms, double* write_ms, double* parse_ms);

#ifdef __cplusplus
}
#endif

#endif /* ADAM_SAM_H */
