// Where a row of a sampler launch reads the Philox stream when the rows are B SEQUENCES x T SUCCESSIVE STEPS (row r = b * T + t: the
// batched sampled lookup step), and how far the accept behind it moves the one counter.  Plain C++ (no HIP; everything is constexpr,
// so device code calls it as it stands): tests/test_host_draw_addr.py compiles this header alone and replays it against the plain
// sampled batched loop, which draws generated id i of sequence b at (c0 + i, b).
//
// The sequences of a batched lookup step run apart: sequence b has emitted steps[b] ids.  There is still ONE counter
// (srgpt_sampling::counter), tied to a definite column of out_ids:
//   m = min over b of max(steps[b], 0)       the column of out_ids every sequence has filled so far;
//   INVARIANT: counter names the draw of column m.  Behind srgpt_llm_sample_first_ex it holds with counter = c0 + 1 and m = 1;
//   row (b, t) fills column max(steps[b], 0) + t of its sequence, so it reads the stream at
//       (counter + (max(steps[b], 0) - m) + t, b)          a 64-bit sum, carried into the high word;
//   the accept moves counter by m_after - m_before (>= 0: no count shrinks; 0 when every sequence is frozen), which keeps the invariant.
// With counter = c0 + m the address is (c0 + steps[b] + t, b): the plain loop's, whatever the steps accepted before.
// Two consequences, pinned by the tests:
//   B = 1: m = steps[0], the address is (counter + t, 0) -- the rows-are-steps mode (pick_draw, pick.h) -- and the advance is the ids
//          the sequence emitted;
//   T = 1 and equal steps[]: the address is (counter, b) -- the sequences-of-one-step mode -- and the advance is one.
#pragma once
#include <stdint.h>

struct DrawAddr {
  uint64_t ctr;  // words 0 and 1 of the Philox counter
  int seq;       // word 2
};

// the ids a sequence has emitted, as the address rule counts them (a negative count is no state of a request: it counts as none)
constexpr int draw_filled(int steps_b) { return steps_b > 0 ? steps_b : 0; }

// m: the column of out_ids every one of the B >= 1 sequences has filled
constexpr int draw_column(const int* steps, int B) {
  int m = draw_filled(steps[0]);
  for (int b = 1; b < B; ++b) m = draw_filled(steps[b]) < m ? draw_filled(steps[b]) : m;
  return m;
}

// row r = b * T + t of a launch over B sequences x T steps, `counter` naming the draw of column draw_column(steps, B)
constexpr DrawAddr draw_addr(uint64_t counter, const int* steps, int B, int T, int r) {
  const int b = r / T, t = r - b * T;
  return DrawAddr{counter + (uint64_t)(draw_filled(steps[b]) - draw_column(steps, B)) + (uint64_t)t, b};
}

// what the accept adds to the counter: the columns that filled up between the steps[] before and after it
constexpr uint64_t draw_advance(int m_before, int m_after) { return m_after > m_before ? (uint64_t)(m_after - m_before) : 0; }
