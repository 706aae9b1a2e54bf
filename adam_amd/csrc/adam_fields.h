// ADAMRecord fields that are a function of a SAM line's FLAG, RNAME, MAPQ and
// RNEXT fields (core/converters/SAMRecordConverter.scala:26-108), shared by
// the ADAM columns (adam_out.hip) and flagstat (flagstat.hip) so that both
// derive them by the same device code.
//
// Uses samk::NameTable / name_lookup / parse_int: include after sam_ingest.hip
// (bqsr_capi.cpp's order).
#ifndef ADAM_FIELDS_H
#define ADAM_FIELDS_H

namespace adamk {

// the FLAG word with 0x400 following the flags column's duplicateRead bit, as
// bqsr_sam_rewrite_quals writes it after MarkDuplicates
__device__ __forceinline__ uint32_t flag_with_dup(uint32_t flag, uint32_t col_flags) {
  return (col_flags & BQSR_F_DUPLICATE) ? (flag | 0x400u) : (flag & ~0x400u);
}

// SAMRecordConverter.scala:72-108: every flag false when the FLAG word is 0;
// the pair flags only for paired reads
__device__ __forceinline__ bool flag_bit(uint32_t f, int k) {
  if (f == 0) return false;
  const bool paired = f & 0x1;
  switch (k) {
    case 0: return paired;                       // readPaired
    case 1: return paired && (f & 0x2);          // properPair
    case 2: return !(f & 0x4);                   // readMapped
    case 3: return paired && !(f & 0x8);         // mateMapped
    case 4: return f & 0x10;                     // readNegativeStrand
    case 5: return paired && (f & 0x20);         // mateNegativeStrand
    case 6: return paired && (f & 0x40);         // firstOfPair
    case 7: return paired && (f & 0x80);         // secondOfPair
    case 8: return !(f & 0x100);                 // primaryAlignment
    case 9: return f & 0x200;                    // failedVendorQualityChecks
    default: return f & 0x400;                   // duplicateRead
  }
}

// referenceId: the @SQ index of RNAME t[a, b), -1 (null) for "*" or a name
// that is no @SQ name (:36-54)
__device__ __forceinline__ int32_t rname_id(const samk::NameTable& sq, const uint8_t* t, int64_t a, int64_t b) {
  if (b - a == 1 && t[a] == '*') return -1;
  return samk::name_lookup(sq, t + a, b - a);
}

// mapq: only when the read has a reference (sq >= 0) and MAPQ != 255
__device__ __forceinline__ bool mapq_field(const uint8_t* t, int64_t a, int64_t b, int32_t sq, int64_t* mapq) {
  *mapq = 255;
  return sq >= 0 && samk::parse_int(t, a, b, mapq) && *mapq != 255;
}

// mateReferenceId (:56-71): RNEXT "=" is RNAME's reference (sq)
__device__ __forceinline__ int32_t rnext_id(const samk::NameTable& sq_tab, const uint8_t* t, int64_t a, int64_t b,
                                            int32_t sq) {
  if (b - a == 1 && t[a] == '=') return sq;
  if (b - a == 1 && t[a] == '*') return -1;
  return samk::name_lookup(sq_tab, t + a, b - a);
}

}  // namespace adamk

#endif  // ADAM_FIELDS_H
