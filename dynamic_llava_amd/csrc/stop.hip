// Device-side stop sequences of generate(stop_sequences= / stopping_criteria=): one launch behind the step-closing launch (dl_decode_advance /
// dl_decode_sample, and behind dl_decode_logprobs when that runs), which has just appended the row's token.  A row that is not finished yet and whose
// generated tokens now END in one of the request's stop sequences gets finished[b] = 1 -- exactly what the step-closing launch does for an EOS token, so
// from the next step on that launch emits pad for the row and the decode loop sees the flag it already observes.  Nothing else is written.
// The rule is dynamic_llava_amd/stopping.py (the contract this kernel is tested against; the reference's KeywordsStoppingCriteria, llava/mm_utils.py:257-267).
//
// One wave per row; the caps (8 sequences of up to 8 tokens) fill its 64 lanes exactly: lane 8 i + j compares position j from the end of sequence i with
// position j from the end of the row.  A lane past its sequence's length votes "equal"; a lane of a sequence that does not take part (past n_stops, longer
// than the row, a length outside 1..8) votes "differs".  One 64-bit ballot then holds a byte per sequence, and sequence i matches iff its byte is 0xff.
// The table and n_stops are device memory the host rewrites between requests: one captured graph serves every stop list.  No LDS, no atomics, no
// workspace, nothing that synchronises with the host; lane 0 stores the flag.
#include "dl_common.h"

namespace dl {

__global__ __launch_bounds__(64) void decode_stop_kernel(const int64_t* __restrict__ out_ids, int out_cap, const int32_t* __restrict__ step,
                                                         int32_t* __restrict__ finished, const dl_stop_table* __restrict__ tab) {
  const int b = blockIdx.x, lane = threadIdx.x, i = lane >> 3, j = lane & 7;
  // uniform over the wave
  if (finished[b] != 0) return;  // a finished row is not touched (its tail is pad from here on)
  const int n = tab->n_stops < DL_STOP_MAX_SEQS ? tab->n_stops : DL_STOP_MAX_SEQS;
  const int s = step[b];
  const int t = s < out_cap ? s : out_cap;  // the row's tokens: out_ids[b, 0 : t]
  if (n <= 0 || t <= 0) return;
  bool vote = false;
  if (i < n) {
    const int len = tab->seq[i][0];
    if (len >= 1 && len <= DL_STOP_MAX_LEN && len <= t)  // (a sequence longer than the row never matches: nothing in front of column 0 is read)
      vote = j >= len || out_ids[(int64_t)b * out_cap + (t - 1 - j)] == (int64_t)tab->seq[i][len - j];  // seq[i][1 + (len - 1 - j)]
  }
  uint64_t m = __ballot(vote);
  m &= m >> 1;
  m &= m >> 2;
  m &= m >> 4;  // bit 8 i: all eight lanes of sequence i voted "equal"
  if (lane == 0 && (m & 0x0101010101010101ull) != 0) finished[b] = 1;
}

}  // namespace dl

using namespace dl;

extern "C" int dl_decode_stop(const int64_t* out_ids, int out_cap, int B, const int32_t* step, int32_t* finished, const dl_stop_table* table, void* stream) {
  DL_REQUIRE(out_ids && step && finished && table, "dl_decode_stop: NULL pointer");
  DL_REQUIRE(B >= 1 && out_cap >= 1, "dl_decode_stop: bad shape B=%d out_cap=%d", B, out_cap);
  hipLaunchKernelGGL(decode_stop_kernel, dim3((unsigned)B), dim3(64), 0, as_stream(stream), out_ids, out_cap, step, finished, table);
  DL_CHECK_LAUNCH("dl_decode_stop");
  return DL_OK;
}
