// cost_emul.cpp -- TEST-ONLY: bce_cost.h compiled by g++ (tests/test_estimate_cpu.py compares it, value by value, with the
// library's build of the same header by hipcc).
#include "../bce_amd/csrc/bce_cost.h"

extern "C" {
uint32_t emul_log2_q24(uint32_t x) { return bce::log2_q24(x); }
uint32_t emul_cost_q24(uint32_t freq, uint32_t total) { return bce::cost_q24(freq, total); }
uint32_t emul_record_cost_q24(uint64_t record) { return bce::record_cost_q24_with(bce::kLog2Table.t, record); }
uint64_t emul_pack_model_out(uint32_t cum, uint32_t freq, uint32_t total, uint32_t esc_word) { return bce::pack_model_out(cum, freq, total, esc_word); }
uint64_t emul_stream_words_q24(uint64_t sum) { return bce::stream_words_q24(sum); }
}
