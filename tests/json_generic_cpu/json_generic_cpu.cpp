// Host build of csrc/json_generic.h (TEST INFRASTRUCTURE): what cep_decode_json runs, record by
// record, for the `-m "not gpu"` tests.  Never linked into libcep.so.
#define __device__
#define __forceinline__ inline
#include "json_generic.h"

#include <vector>

extern "C" void jg_pow5(uint64_t* out) { cep::jsong::build_pow5_table(out); }

// cep_decode_json on host memory; the argument-check message or NULL
extern "C" const char* jg_decode(const uint8_t* bytes, const uint64_t* rec_off, uint64_t n,
                                 const cep_json_field* fields, uint32_t n_fields, void* const* cols,
                                 const char* span_field, uint32_t* span, int32_t* status) {
  static std::vector<uint64_t> pow5;
  if (pow5.empty()) {
    pow5.resize(2 * cep::jsong::kPow5Count);
    cep::jsong::build_pow5_table(pow5.data());
  }
  cep::jsong::Table tab;
  if (const char* msg = cep::jsong::fill_table(&tab, fields, n_fields, cols, span_field)) return msg;
  for (uint64_t r = 0; r < n; r++)
    status[r] = cep::jsong::decode_record(bytes + rec_off[r], (uint32_t)(rec_off[r + 1] - rec_off[r]), &tab,
                                          pow5.data(), r, span_field ? span : nullptr);
  return nullptr;
}
