// TEST-ONLY: siddhi_amd/csrc/gw_proj.h (k_gtile_count, k_gscan_project<RPT> and their launches) compiled for the CPU
// (SG_HOST_ONLY over simt_shim.h) as a stand-alone program for -fsanitize=address,undefined: tests/
// test_group_walk_project_host.py builds and runs it.  Every buffer has exactly the size run_group_walk gives it
// (trigger words: n; match area: 3 units per row + GW_AREA_PAD; records: the push's matches), so a read or a store
// past one is reported, and the records are compared with a serial projection of the same words.
//
// Cases, each for RPT 1, 2, 4, select lists of 1 and 4 columns and out_base 0 (no index column) and 1 (an index
// column of exactly n words):
//   dense   64 keys in turn, every row but a key's first completes one partial: every row of the tiles after the
//           first is a trigger, the LDS list is at its bound
//   end     random triggers of 0..3 matches, stale words of another epoch on the rows that trigger nothing, one
//           trigger of 300 matches at a tile's last row, and the highest key's last row -- the batch's last row --
//           triggering m = 1, 2, 3 matches: its header and entries are the last used units of the match area
#define SG_HOST_ONLY 1
#include "simt_shim.h"

#include "../../siddhi_amd/csrc/gw_proj.h"

#include <cstring>
#include <map>
#include <random>

namespace {

struct Push {
  int64_t n = 0;
  uint32_t epoch = 3;
  std::vector<uint32_t> key, want;   // per row: its key, the matches it should complete if the key holds as many
  std::vector<uint64_t> trig, area;
  std::vector<uint32_t> m;           // matches per row as laid out
  uint32_t total = 0;
};

// the walker's layout: keys in id order, 3 units per row of the key; per trigger a 2-unit header and its entries
void lay_out(Push& p, std::mt19937& rng) {
  const int64_t n = p.n;
  std::map<uint32_t, std::vector<int64_t>> rows;
  for (int64_t b = 0; b < n; ++b) rows[p.key[b]].push_back(b);
  p.trig.assign((size_t)n, 0);
  p.m.assign((size_t)n, 0);
  p.area.assign((size_t)(3 * n + GW_AREA_PAD), 0xdeadbeefdeadbeefull);
  uint64_t base = 0;
  for (auto& kv : rows) {
    uint64_t cur = base;
    uint32_t pending = 0;
    for (int64_t b : kv.second) {
      const uint32_t m = std::min(p.want[b], pending);
      if (m) {
        p.area[cur] = (uint64_t)(uint32_t)(1000 + b) | ((uint64_t)kv.first << 32);
        p.area[cur + 1] = (uint64_t)(uint32_t)rng() | ((uint64_t)(uint32_t)rng() << 32);
        for (uint32_t q = 0; q < m; ++q) p.area[cur + 2 + q] = (uint64_t)(uint32_t)rng() | ((uint64_t)(uint32_t)rng() << 32);
        p.trig[b] = gw_trig_word(cur, m, p.epoch);
        p.m[b] = m;
        p.total += m;
        cur += 2 + m;
        pending -= m;
      } else {
        p.trig[b] = gw_trig_word(rng() % (3 * n), 1 + rng() % 5, p.epoch - 1 - rng() % 2);   // stale: another epoch
      }
      ++pending;
    }
    base += 3 * kv.second.size();
    if (cur > base) abort();
  }
}

GwSel select_of(int nsel) {
  GwSel s;
  memset(&s, 0, sizeof(s));
  s.n_select = nsel;
  s.stride = 32 + 8 * nsel;
  s.vfloat = 1;
  for (int c = 0; c < nsel; ++c) s.codes[0] |= (uint64_t)(c & 3) << (4 * c);
  return s;
}

std::vector<int64_t> reference(const Push& p, const GwSel& s, int64_t t0, uint64_t base_index, const uint64_t* index) {
  std::vector<int64_t> out;
  auto wid = [](uint32_t bits, bool zero) { return zero ? (int64_t)bits : (int64_t)(int32_t)bits; };
  for (int64_t b = 0; b < p.n; ++b) {
    const uint64_t u = (uint32_t)p.trig[b];
    for (uint32_t q = 0; q < p.m[b]; ++q) {
      const uint64_t h0 = p.area[u], h1 = p.area[u + 1], e = p.area[u + 2 + q];
      out.push_back((int64_t)(index ? index[b] : base_index + (uint64_t)b));
      out.push_back(t0 + (int64_t)(int32_t)(uint32_t)h0);
      out.push_back((int64_t)((h0 >> 32) | ((uint64_t)((1u << 24) | 0x800000u | q) << 32)));
      out.push_back((int64_t)s.nmask);
      const int64_t col[4] = {wid((uint32_t)(e >> 32), s.pzero), wid((uint32_t)e, s.vfloat), wid((uint32_t)h1, s.vfloat),
                              wid((uint32_t)(h1 >> 32), s.pzero)};
      for (int c = 0; c < s.n_select; ++c) out.push_back(col[(s.codes[0] >> (4 * c)) & 15u]);
    }
  }
  return out;
}

int run(const char* name, const Push& p) {
  int bad = 0;
  for (int rpt : {1, 2, 4})
    for (int nsel : {1, 4})
      for (int64_t out_base : {(int64_t)0, (int64_t)1}) {
        char env[8];
        snprintf(env, sizeof(env), "%d", rpt);
        setenv("SG_DEBUG_GW_PROJ_RPT", env, 1);
        if (gw_proj_rpt() != rpt) abort();
        const uint32_t lg = gw_proj_lg_tile(rpt);
        const int64_t ntile = (p.n + ((int64_t)1 << lg) - 1) >> lg;
        std::vector<uint32_t> tcount((size_t)ntile + 1, 0), tbase((size_t)ntile + 1, 0);
        launch_gtile_count(p.n, p.trig.data(), p.epoch, tcount.data(), ntile, lg, nullptr);
        for (int64_t i = 0; i < ntile; ++i) {
          uint32_t c = 0;
          for (int64_t b = i << lg; b < std::min(p.n, (i + 1) << lg); ++b) c += p.m[b];
          if (c != tcount[i]) { ++bad; fprintf(stderr, "%s rpt %d: tile %lld counts %u, not %u\n", name, rpt, (long long)i, tcount[i], c); }
          tbase[i + 1] = tbase[i] + tcount[i];
        }
        const GwSel s = select_of(nsel);
        const int64_t t0 = 1700000000000ll;
        const uint64_t base_index = 12345;
        std::vector<char> out((size_t)(out_base + p.total) * s.stride, (char)0x5a);
        // with out_base 1 the batch carries an index column of exactly n words: the trigger is index[b] of the entry's row
        std::vector<uint64_t> index_col;
        if (out_base)
          for (int64_t b = 0; b < p.n; ++b) index_col.push_back(7 + 3 * (uint64_t)b);
        const uint64_t* index = out_base ? index_col.data() : nullptr;
        launch_gscan_project(rpt, p.n, t0, base_index, index, p.trig.data(), p.epoch, p.area.data(), s, ntile, out_base,
                             out.data(), tbase.data(), nullptr);
        const std::vector<int64_t> want = reference(p, s, t0, base_index, index);
        if (want.size() * 8 != (size_t)p.total * s.stride) abort();
        if (memcmp(out.data() + out_base * s.stride, want.data(), want.size() * 8) != 0) {
          ++bad;
          fprintf(stderr, "%s rpt %d nsel %d out_base %lld: records differ\n", name, rpt, nsel, (long long)out_base);
        }
        for (int64_t x = 0; x < out_base * s.stride; ++x)
          if (out[x] != (char)0x5a) { ++bad; fprintf(stderr, "%s: bytes before out_base written\n", name); break; }
      }
  printf("%s: n %lld, matches %u, %s\n", name, (long long)p.n, p.total, bad ? "FAILED" : "ok");
  return bad;
}

Push dense(int64_t n) {
  std::mt19937 rng(5);
  Push p;
  p.n = n;
  for (int64_t b = 0; b < n; ++b) {
    p.key.push_back(1000 + 997 * (uint32_t)(b % 64));
    p.want.push_back(1);
  }
  lay_out(p, rng);
  if (p.total != n - 64) abort();
  return p;
}

Push end_of_area(int64_t n, uint32_t m_last) {
  std::mt19937 rng(7 + m_last);
  Push p;
  p.n = n;
  const uint32_t top = 70000, deep = 500;
  for (int64_t b = 0; b < n; ++b) {
    p.key.push_back(1 + 700 * (uint32_t)(rng() % 40));
    p.want.push_back(rng() % 10 < 3 ? 1 + rng() % 3 : 0);
  }
  // 300 rows of `deep` that complete nothing, then one that completes them all, at the last row of a 1024-row tile
  for (int64_t j = 0; j <= 300; ++j) {
    const int64_t b = 1023 - 2 * (300 - j);
    p.key[b] = deep;
    p.want[b] = j == 300 ? 300 : 0;
  }
  for (uint32_t j = 0; j <= m_last; ++j) {
    const int64_t b = n - 1 - 3 * (int64_t)(m_last - j);
    p.key[b] = top;
    p.want[b] = j == m_last ? m_last : 0;
  }
  lay_out(p, rng);
  if (p.m[1023] != 300 || p.m[n - 1] != m_last) abort();
  // the last trigger's last entry is the last used unit of the area
  const uint64_t u = (uint32_t)p.trig[n - 1];
  for (int64_t b = 0; b < n; ++b)
    if (p.m[b] && (uint32_t)p.trig[b] > u) abort();
  return p;
}

}   // namespace

int main() {
  int bad = 0;
  bad += run("dense", dense(3 * 1024));
  for (uint32_t m : {1u, 2u, 3u}) {
    char name[32];
    snprintf(name, sizeof(name), "end_m%u", m);
    bad += run(name, end_of_area(2 * 1024 + 5, m));
  }
  return bad ? 1 : 0;
}
