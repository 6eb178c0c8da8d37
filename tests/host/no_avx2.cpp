// Linked in place of csrc/sampler_x86.cpp: the CPU check answers "no AVX2", so walk_stream, temper_block and mt_twist of
// csrc/sampler.cpp take their scalar fall-backs.  The vector entry points must then never be reached.
#include <cstdint>
#include <cstdlib>

extern "C" {
int ggad_x86_has_avx2(void) { return 0; }
int ggad_x86_accept8(const uint32_t *, int, uint32_t, int32_t *) { std::abort(); }
int ggad_x86_accept_run(const uint32_t *, int, int64_t, int64_t *, int32_t *) { std::abort(); }
void ggad_x86_temper(const uint32_t *, uint32_t *, int) { std::abort(); }
void ggad_x86_mt_twist(uint32_t *) { std::abort(); }
}
