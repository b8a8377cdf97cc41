// CPU-only checker of the per-layer layered decoder's compaction of running codewords (compact_wanted, compact_rank,
// compact_tile_count, compact_done_word, pass_compact_bytes of
// informationbottleneckdecodingldpc_amd/csrc/layered_plan.h), built by tests/test_cpu_layered_compact.py with
// -fsanitize=address,undefined -fno-sanitize-recover=all.
//
//   layered_compact_plan_check [decode.bin]
// Always: the header's predicate and rank map against brute force on adversarial and random finished masks (all
// running, all finished, one survivor in the last column, survivors only in the last tile, batches of 1, 63, 64, 65,
// 130, 260 and more, with the padding bits of the last tile set as the kernels keep them); the chunked in-place
// move (load a chunk, then store it, chunks ascending) replayed sequentially for several chunk sizes against an
// out-of-place gather; every index against pass_compact_bytes and the row length. The maps are formed the way
// lay_compact_plan forms them (a scan over chunks of 64 tiles), the move the way lay_compact_rows and
// lay_compact_commit make it.
// With decode.bin (int32 B, imax, every, min_free_pct, iters[B]: the reference's iteration counts): replays the
// masks of that decode through the same functions — stage-in, the stop check of iterations 1 .. imax - 1, an attempt
// after every `every`-th — and prints the compactions it decided.
// One JSON line {events: [[it, E, R], ...], extent, orig: [...], cases, failures}; exit status 0 = every invariant held.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "layered_plan.h"

using namespace ibl;

static int g_fail = 0;
static long g_cases = 0;
#define CHECK(cond, what)                                               \
  do {                                                                  \
    if (!(cond)) {                                                      \
      if (g_fail < 20) std::fprintf(stderr, "invariant failed: %s (%s)\n", what, #cond); \
      ++g_fail;                                                         \
    }                                                                   \
  } while (0)

struct State {
  int32_t B = 0, ldb = 0, ntiles = 0, extent = 0, running = 0, count = 0;
  std::vector<uint64_t> done;     // [ntiles]
  std::vector<int32_t> orig, dest;   // sized by pass_compact_bytes
  std::vector<int32_t> row;       // [ldb] one row of P: holds the caller's column of the codeword it belongs to
  std::vector<int32_t> out;       // [B] the caller's row; -1 = not delivered
  std::vector<int32_t> delivered; // [B] times written
};

static bool is_done(const State& s, int32_t c) { return (s.done[(size_t)c / kLayTile] >> (c % kLayTile)) & 1ull; }

static void stage_in(State* s, int32_t B) {
  s->B = B;
  s->ntiles = pass_tiles(B);
  s->ldb = (int32_t)pass_ldb(B);
  const LayeredCompactBytes by = pass_compact_bytes(B);
  CHECK(by.orig == (size_t)4 * s->ldb && by.dest == by.orig && by.ctl == (size_t)4 * kLayCompactCtl &&
            by.total == by.orig + by.dest + by.ctl, "compaction state bytes");
  s->orig.assign(by.orig / 4, -7);
  s->dest.assign(by.dest / 4, -7);
  s->done.assign((size_t)s->ntiles, 0ull);
  s->row.assign((size_t)s->ldb, -1);
  s->out.assign((size_t)B, -1);
  s->delivered.assign((size_t)B, 0);
  for (int32_t t = 0; t < s->ntiles; ++t) {
    const int32_t left = B - t * kLayTile;
    s->done[t] = left >= kLayTile ? 0ull : ~0ull << left;
    CHECK(s->done[t] == compact_done_word(t, B), "stage-in's padding is the done word of an extent of B");
  }
  for (int32_t c = 0; c < s->ldb; ++c) s->orig[c] = c;
  for (int32_t c = 0; c < B; ++c) s->row[c] = c;
  s->extent = s->running = B;
  s->count = 0;
}

// brute force, nothing shared with the header
static bool brute_wanted(int32_t R, int32_t E, int32_t pct) {
  if (R <= 0) return false;
  int32_t tE = 0, tR = 0;
  for (int32_t c = 0; c < E; c += kLayTile) ++tE;
  for (int32_t c = 0; c < R; c += kLayTile) ++tR;
  int32_t need = 0;
  while ((int64_t)100 * need < (int64_t)pct * tE) ++need;
  if (need < 1) need = 1;
  return tE - tR >= need;
}

// dest[0 .. E) as lay_compact_plan: chunks of 64 tiles, an exclusive scan of the tile counts, compact_rank per column
static void plan(State* s) {
  const int32_t E = s->extent, tE = pass_tiles(E);
  CHECK(tE <= s->ntiles, "the extent's tiles are within the masks");
  int32_t below = 0;
  for (int32_t t0 = 0; t0 < tE; t0 += 64) {
    int32_t excl[64], inc = 0;
    uint64_t dm[64];
    for (int j = 0; j < 64; ++j) {
      dm[j] = t0 + j < tE ? s->done[(size_t)t0 + j] : ~0ull;
      excl[j] = below + inc;
      inc += compact_tile_count(dm[j]);
    }
    for (int j = 0; j < 64 && t0 + j < tE; ++j)
      for (int lane = 0; lane < kLayTile; ++lane) {
        const int32_t col = (t0 + j) * kLayTile + lane;
        if (col >= E) continue;
        CHECK((size_t)col < s->dest.size(), "dest index within its buffer");
        s->dest[col] = compact_rank(dm[j], lane, excl[j]);
      }
    below += inc;
  }
  // against brute force
  int32_t r = 0;
  for (int32_t c = 0; c < E; ++c) {
    const int32_t want = is_done(*s, c) ? -1 : r;
    CHECK(s->dest[c] == want, "rank map");
    CHECK(s->dest[c] <= c, "the map is stable: no column moves up");
    if (want >= 0) ++r;
  }
  CHECK(r == s->running && below == r, "the masks hold `running` clear bits below the extent");
  for (int32_t c = E; c < s->ldb; ++c) CHECK(is_done(*s, c), "every column past the extent is finished");
}

// the row move of lay_compact_rows on the one row, chunk columns at a time, and the commit
static void move_and_commit(State* s, int32_t chunk) {
  const int32_t E = s->extent, R = s->running;
  // out of place: what the row and orig must be afterwards
  std::vector<int32_t> want_row, want_orig;
  for (int32_t c = 0; c < E; ++c)
    if (!is_done(*s, c)) {
      want_row.push_back(s->row[c]);
      want_orig.push_back(s->orig[c]);
    }
  std::vector<int32_t> x((size_t)chunk), o((size_t)chunk);
  for (int32_t c0 = 0; c0 < E; c0 += chunk) {
    const int32_t n = E - c0 < chunk ? E - c0 : chunk;
    for (int32_t i = 0; i < n; ++i) x[i] = s->row[(size_t)c0 + i];   // load the chunk
    for (int32_t i = 0; i < n; ++i) {                                // then store it
      const int32_t c = c0 + i, d = s->dest[c];
      if (d >= 0) {
        CHECK(d < R && d <= c0 + n - 1, "a destination lies at or below the chunk's last source");
        s->row[(size_t)d] = x[i];
      } else {
        const int32_t b = s->orig[c];
        CHECK(b >= 0 && b < s->B, "a flushed codeword's column is the caller's");
        if (b >= 0 && b < s->B) {
          s->out[b] = x[i];
          ++s->delivered[b];
        }
      }
    }
  }
  for (int32_t c0 = 0; c0 < E; c0 += chunk) {   // orig, by the same rule
    const int32_t n = E - c0 < chunk ? E - c0 : chunk;
    for (int32_t i = 0; i < n; ++i) o[i] = s->orig[(size_t)c0 + i];
    for (int32_t i = 0; i < n; ++i)
      if (s->dest[c0 + i] >= 0) s->orig[(size_t)s->dest[c0 + i]] = o[i];
  }
  CHECK((int32_t)want_row.size() == R, "running columns");
  for (int32_t c = 0; c < R && c < (int32_t)want_row.size(); ++c) {
    CHECK(s->row[c] == want_row[c], "in place equals the out-of-place gather (row)");
    CHECK(s->orig[c] == want_orig[c], "in place equals the out-of-place gather (orig)");
    CHECK(s->row[c] == s->orig[c], "a column holds the codeword orig names");
  }
  const int32_t tE = pass_tiles(E);
  for (int32_t t = 0; t < tE; ++t) s->done[t] = compact_done_word(t, R);
  for (int32_t c = 0; c < s->ldb; ++c) CHECK(is_done(*s, c) == (c >= R), "finished exactly from column R on");
  for (int32_t t = pass_tiles(R); t < s->ntiles; ++t) CHECK(s->done[t] == ~0ull, "tiles past the running ones are all ones");
  s->extent = R;
  ++s->count;
}

// lay_stage_out_c, then: every codeword reached the caller exactly once, with its own values
static void stage_out(State* s) {
  for (int32_t c = 0; c < s->extent; ++c) {
    const int32_t b = s->orig[c];
    CHECK(b >= 0 && b < s->B, "orig within the batch");
    if (b >= 0 && b < s->B) {
      s->out[b] = s->row[c];
      ++s->delivered[b];
    }
  }
  for (int32_t b = 0; b < s->B; ++b) CHECK(s->delivered[b] == 1 && s->out[b] == b, "each codeword delivered once, unmixed");
}

// one mask: finish the columns `fin` of a fresh batch, attempt a compaction, then a second one on what is left
static void one_mask(int32_t B, const std::vector<char>& fin, int32_t pct, int32_t chunk, std::mt19937* rng) {
  ++g_cases;
  State s;
  stage_in(&s, B);
  for (int round = 0; round < 2; ++round) {
    for (int32_t c = 0; c < s.extent; ++c) {
      const bool f = round == 0 ? fin[(size_t)s.orig[c]] != 0 : !is_done(s, c) && ((*rng)() & 1u);
      if (f && !is_done(s, c)) {
        s.done[(size_t)c / kLayTile] |= 1ull << (c % kLayTile);
        --s.running;
      }
    }
    const bool want = compact_wanted(s.running, s.extent, pct);
    CHECK(want == brute_wanted(s.running, s.extent, pct), "predicate");
    if (!want) continue;
    plan(&s);
    move_and_commit(&s, chunk);
  }
  stage_out(&s);
}

int main(int argc, char** argv) {
  std::mt19937 rng(12345);
  // the predicate alone, over every (R, E) of a few tiles and the percentages' edges
  for (int32_t E = 1; E <= 6 * kLayTile + 1; ++E)
    for (int32_t R = 0; R <= E; ++R)
      for (int32_t pct : {1, 12, 25, 33, 50, 99, 100})
        CHECK(compact_wanted(R, E, pct) == brute_wanted(R, E, pct), "predicate, exhaustive");
  CHECK(!compact_wanted(0, 8192, 1) && compact_wanted(1, 65, 50) && !compact_wanted(1, 65, 100) &&
            !compact_wanted(65, 128, 1) && compact_wanted(64, 128, 50), "predicate, spot");
  CHECK(compact_wanted(1, 0x7fffffff, 99) && !compact_wanted(0x7fffffff, 0x7fffffff, 1), "predicate, no overflow");
  for (int32_t B : {1, 63, 64, 65, 130, 260, 4097 + 64 * 64}) {
    std::vector<std::vector<char>> masks;
    std::vector<char> m((size_t)B, 0);
    masks.push_back(m);                                    // all running
    masks.push_back(std::vector<char>((size_t)B, 1));      // all finished
    m.assign((size_t)B, 1); m[(size_t)B - 1] = 0;
    masks.push_back(m);                                    // one survivor, in the last column
    m.assign((size_t)B, 1);
    for (int32_t c = (B - 1) / kLayTile * kLayTile; c < B; ++c) m[c] = 0;
    masks.push_back(m);                                    // survivors only in the last tile
    m.assign((size_t)B, 0);
    for (int32_t c = 0; c < B && c < kLayTile; ++c) m[c] = 1;
    masks.push_back(m);                                    // the first tile finished
    m.assign((size_t)B, 0);
    for (int32_t c = 0; c < B; c += 2) m[c] = 1;
    masks.push_back(m);                                    // every second column
    m.assign((size_t)B, 1); m[0] = 0;
    masks.push_back(m);                                    // one survivor, in place already
    for (int density : {2, 8, 50, 92, 98})
      for (int rep = 0; rep < 3; ++rep) {
        for (int32_t c = 0; c < B; ++c) m[c] = (int)(rng() % 100) < density;
        masks.push_back(m);
      }
    for (const auto& mask : masks)
      for (int32_t pct : {1, 50, 100})
        for (int32_t chunk : {1, 3, 64, 256, 1000}) one_mask(B, mask, pct, chunk, &rng);
  }

  std::string events, origs;
  int32_t extent = 0;
  if (argc == 2) {
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[4];
    if (std::fread(hdr, 4, 4, f) != 4) return 2;
    const int32_t B = hdr[0], imax = hdr[1], every = hdr[2], pct = hdr[3];
    if (B < 1 || imax < 1 || every < 1 || pct < 1 || pct > 100) return 2;
    std::vector<int32_t> iters((size_t)B);
    if (std::fread(iters.data(), 4, (size_t)B, f) != (size_t)B) return 2;
    std::fclose(f);
    State s;
    stage_in(&s, B);
    for (int32_t it = 1; it < imax; ++it) {
      for (int32_t c = 0; c < s.extent; ++c)   // lay_finalise_c(it)
        if (!is_done(s, c) && iters[(size_t)s.orig[c]] == it) {
          s.done[(size_t)c / kLayTile] |= 1ull << (c % kLayTile);
          --s.running;
        }
      if (it % every || !compact_wanted(s.running, s.extent, pct)) continue;
      events += (events.empty() ? "[" : ", [") + std::to_string(it) + ", " + std::to_string(s.extent) + ", " +
                std::to_string(s.running) + "]";
      plan(&s);
      move_and_commit(&s, 4 * kLayTile);
    }
    extent = s.extent;
    for (int32_t c = 0; c < extent; ++c) origs += (c ? ", " : "") + std::to_string(s.orig[c]);
    stage_out(&s);
  } else if (argc != 1) {
    std::fprintf(stderr, "usage: layered_compact_plan_check [decode.bin]\n");
    return 2;
  }
  std::printf("{\"events\": [%s], \"extent\": %d, \"orig\": [%s], \"cases\": %ld, \"failures\": %d}\n", events.c_str(),
              extent, origs.c_str(), g_cases, g_fail);
  return g_fail ? 1 : 0;
}
