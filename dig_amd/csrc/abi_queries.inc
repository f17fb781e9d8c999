// The host-only queries of the C ABI (include/dig_hip.h) whose answer is the same in both builds, defined once: each forwards to the
// inline function of abi_rules.h that the argument rules and the launchers use, so a query, the rule that holds a caller to its answer and
// the launcher cannot drift apart.  Included by csrc/abi_queries.hip (HIP build) and cpu_abi/dig_cpu.cpp (plain-C++ build).  Needs
// abi_rules.h, <algorithm> and <vector>.  (dig_bn_stats_workspace_bytes and dig_colsum_workspace_bytes describe their own build's
// partial-sum layout and stay per build.)
// Number of R-splits dig_gemm_bf16 will really use for a requested split count (slabs are whole 64-row K-tiles).
extern "C" int dig_gemm_effective_splits(int R, int splits) { return dig_rules::gemm_effective_splits(R, splits); }

extern "C" int dig_wgrad_group_supported(int I, int J, int R) { return dig_rules::wgrad_group_supported(I, J, R); }
extern "C" int dig_wgrad_group_fn(int J) { return dig_rules::wgrad_group_fn(J); }
extern "C" int dig_wgrad_group_rows_per_split(int R, int splits) { return dig_rules::wgrad_group_rows_per_split(R, splits); }
extern "C" int dig_wgrad_group_effective_splits(int R, int splits) { return dig_rules::wgrad_group_effective_splits(R, splits); }
extern "C" long long dig_wgrad_group_slab_bytes(int total_tiles, int splits, int fn, int wa) { return dig_rules::wgrad_group_slab_bytes(total_tiles, splits, fn, wa); }
extern "C" int dig_wgrad_group_tiles(int I, int J, int fn, int wa) { return dig_rules::wgrad_group_tiles(I, J, fn, wa); }

extern "C" int dig_layernorm_bwd_parts(int rows) { return dig_rules::layernorm_bwd_parts(rows); }
extern "C" long long dig_layernorm_bwd_workspace_bytes(int rows, int D) { return dig_rules::layernorm_bwd_workspace_bytes(rows, D); }
extern "C" int dig_bn_fused_supported(int rows, int C) { return dig_rules::bn_fused_supported(rows, C); }
extern "C" int dig_attn_block_supported(int heads, int embed_dim) { return dig_rules::attn_block_supported(heads, embed_dim); }
extern "C" int dig_mlp_chain_supported(int D, int F) { return dig_rules::mlp_chain_supported(D, F); }
extern "C" int dig_mlp_chain_ln_parts(int R) { return dig_rules::mlp_chain_ln_parts(R); }
extern "C" int dig_mlp_chain_colsum_rows(int R) { return dig_rules::mlp_chain_colsum_rows(R); }
extern "C" long long dig_lexicon_search_workspace_bytes(int B, int max_count) { return dig_rules::lexicon_search_workspace_bytes(B, max_count); }
extern "C" long long dig_ctc_lexicon_workspace_bytes(int B, int T, int C, int max_count) { return dig_rules::ctc_lexicon_workspace_bytes(B, T, C, max_count); }
extern "C" long long dig_sumsq_workspace_bytes(long long n) { return dig_rules::sumsq_workspace_bytes(n); }
extern "C" long long dig_mse_workspace_bytes() { return dig_rules::mse_workspace_bytes(); }
extern "C" long long dig_ce_rows_workspace_bytes(int n) { return dig_rules::ce_rows_workspace_bytes(n); }
extern "C" long long dig_tcv_attn_bwd_workspace_bytes(int S, int Lq, int heads, int d) { return dig_rules::tcv_attn_bwd_workspace_bytes(S, Lq, heads, d); }

// Workgroup table of one launch (host memory in, host memory out): tiles_per_prob[n_probs] tiles x S R-splits, the tiles of one
// (problem, split) pair on one XCD, the eight XCDs loaded evenly.  S = the largest split count <= max_wg / tiles (whole groups of
// four 16-row stages per split) whose table fits max_wg workgroups (one round at two workgroups per CU: 512 on MI355X); *splits_out
// receives it.  map_out[n_wg] entries: tile | split << 16, or 0xffffffff (a workgroup that only takes part in the fold).
// Returns n_wg (a multiple of 8, <= max_out) or a negative error.
extern "C" int dig_wgrad_group_plan(const int* tiles_per_prob, int n_probs, int R, int max_wg, int* splits_out, unsigned* map_out,
                                    int max_out) {
  if (!tiles_per_prob || !map_out || !splits_out || n_probs < 1 || n_probs > DIG_WGRAD_MAX_PROBS || R < 64 || (R % 64) || max_wg < 8) return DIG_ERR_ARG;
  int tiles = 0;
  for (int k = 0; k < n_probs; ++k) {
    if (tiles_per_prob[k] < 1) return DIG_ERR_ARG;
    tiles += tiles_per_prob[k];
  }
  if (tiles > 65535) return DIG_ERR_ARG;
  struct Grp { int tile0, n, split; };
  int last_eff = -1;
  for (int want = std::max(1, std::min(max_wg / tiles, R / 64));; --want) {
    const int S = dig_rules::wgrad_group_effective_splits(R, want);
    if (S == last_eff && want > 1) continue;
    last_eff = S;
    std::vector<Grp> groups;
    int tile0 = 0;
    for (int k = 0; k < n_probs; ++k) {
      for (int s = 0; s < S; ++s) groups.push_back({tile0, tiles_per_prob[k], s});
      tile0 += tiles_per_prob[k];
    }
    std::stable_sort(groups.begin(), groups.end(), [](const Grp& a, const Grp& b) { return a.n > b.n; });
    std::vector<unsigned> bins[8];
    for (const Grp& g : groups) {
      int best = 0;
      for (int x = 1; x < 8; ++x)
        if (bins[x].size() < bins[best].size()) best = x;
      for (int t = 0; t < g.n; ++t) bins[best].push_back((unsigned)(g.tile0 + t) | ((unsigned)g.split << 16));
    }
    size_t len = 0;
    for (int x = 0; x < 8; ++x) len = std::max(len, bins[x].size());
    if ((long long)len * 8 > max_wg && want > 1) continue;
    if ((long long)len * 8 > max_out || S > 65535) return DIG_ERR_ARG;
    for (size_t k = 0; k < len; ++k)
      for (int x = 0; x < 8; ++x) map_out[k * 8 + x] = k < bins[x].size() ? bins[x][k] : 0xffffffffu;
    *splits_out = S;
    return (int)(len * 8);
  }
}
