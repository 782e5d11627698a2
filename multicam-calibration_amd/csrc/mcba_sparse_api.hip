// mcba_sparse_api.hip -- host side of the sparse-Schur handle (mcba_create_sparse): the visibility index, the buffers it sizes, and the
// launch sequences that replace k_syrk + k_reduce_system's tile pairs and k_solve_cam on such a handle (kernels: mcba_sparse.hip).
#include "mcba_handle.h"

namespace mcba_internal {

// chunk length of a co-visible pair's frame list: a diagonal pair carries every frame of its camera, so the long lists are cut here and
// the chunk sums are added in chunk order by k_sp_assemble
constexpr int kSpChunk = 64;

// The visibility index, from seen[c * F + f] (camera c has a detection in frame f): which cameras saw each frame (entries, frame-major,
// cameras ascending), the co-visible pairs (i <= j, ordered by (i, j)) with the frames both saw in ascending order, and their chunks.
// O(sum_f k_f^2) for k_f cameras in frame f, plus a C x C pair map.  Pure host code: mcba_sparse_index exposes it.
struct SpIndex {
  std::vector<int> frame_off, ent_cam, ent_frame, items, chunks, pair_map, pair_chunks;
  int npairs = 0;
};
static void build_index(const unsigned char* seen, int C, int F, SpIndex& x) {
  x.frame_off.assign(F + 1, 0);
  x.ent_cam.clear(); x.ent_frame.clear();
  for (int f = 0; f < F; ++f) {
    for (int c = 0; c < C; ++c)
      if (seen[(size_t)c * F + f]) { x.ent_cam.push_back(c); x.ent_frame.push_back(f); }
    x.frame_off[f + 1] = (int)x.ent_cam.size();
  }
  const std::vector<int>& frame_off = x.frame_off;
  const std::vector<int>& ent_cam = x.ent_cam;
  // pairs: count, number in (i, j) order, fill in frame order
  std::vector<int>& pair_map = x.pair_map;
  pair_map.assign((size_t)C * C, -1);
  std::vector<int> cnt((size_t)C * C, 0);
  for (int f = 0; f < F; ++f)
    for (int a = frame_off[f]; a < frame_off[f + 1]; ++a)
      for (int b = a; b < frame_off[f + 1]; ++b) ++cnt[(size_t)ent_cam[a] * C + ent_cam[b]];
  std::vector<int> pair_start;
  int npairs = 0;
  size_t nitems = 0;
  for (size_t ij = 0; ij < (size_t)C * C; ++ij)
    if (cnt[ij]) { pair_map[ij] = npairs++; pair_start.push_back((int)nitems); nitems += cnt[ij]; }
  pair_start.push_back((int)nitems);
  x.items.assign(3 * nitems, 0);
  std::vector<int> fill(pair_start.begin(), pair_start.end() - 1);
  for (int f = 0; f < F; ++f)
    for (int a = frame_off[f]; a < frame_off[f + 1]; ++a)
      for (int b = a; b < frame_off[f + 1]; ++b) {
        const int p = pair_map[(size_t)ent_cam[a] * C + ent_cam[b]];
        int* it = &x.items[3 * (size_t)fill[p]++];
        it[0] = a; it[1] = b; it[2] = f;
      }
  x.chunks.clear();
  x.pair_chunks.assign(npairs + 1, 0);
  for (int i = 0, p = 0; i < C; ++i)
    for (int j = i; j < C; ++j) {
      if (pair_map[(size_t)i * C + j] < 0) continue;
      for (int s = pair_start[p]; s < pair_start[p + 1]; s += kSpChunk) {
        x.chunks.push_back(s);
        x.chunks.push_back(std::min(kSpChunk, pair_start[p + 1] - s));
        x.chunks.push_back(i == j ? 1 : 0);
      }
      x.pair_chunks[++p] = (int)x.chunks.size() / 3;
    }
  x.npairs = npairs;
}

// the index of the uploaded observations, built once per upload
static int sparse_index(mcba_handle* h) {
  if (h->sp_ready) return MCBA_OK;
  const int C = h->C, F = h->F;
  int rc;
  std::vector<unsigned char> seen((size_t)C * F);
  {
    unsigned char* d_seen = nullptr;
    HIPCHK(pool_malloc(reinterpret_cast<void**>(&d_seen), seen.size(), h->device, h->stream));
    mcba::launch_sp_seen(h->stream, h->obs_raw, d_seen, C, F, h->N);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(seen.data(), d_seen, seen.size(), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    pool_free(d_seen, seen.size(), h->device, h->stream);
    if (e != hipSuccess) { g_err = std::string("sparse visibility index: ") + hipGetErrorString(e); return MCBA_ERR_HIP; }
  }
  SpIndex x;
  build_index(seen.data(), C, F, x);
  const std::vector<int> &frame_off = x.frame_off, &ent_cam = x.ent_cam, &ent_frame = x.ent_frame, &items = x.items, &chunks = x.chunks, &pair_map = x.pair_map,
                         &pair_chunks = x.pair_chunks;
  const int nent = (int)ent_cam.size(), npairs = x.npairs, nchunks = (int)chunks.size() / 3;
  // one int arena on the device: frame_off | ent_cam | ent_frame | items | chunks | pair_map | pair_chunks
  std::vector<int> arena;
  size_t off[8];
  auto put = [&](int k, const std::vector<int>& v) { off[k] = arena.size(); arena.insert(arena.end(), v.begin(), v.end()); arena.resize((arena.size() + 63) / 64 * 64); };
  put(0, frame_off); put(1, ent_cam); put(2, ent_frame); put(3, items); put(4, chunks); put(5, pair_map); put(6, pair_chunks);
  if (arena.size() > h->sp_index_ints) {
    if (h->sp_index) {
      for (size_t i = 0; i < h->bufs.size(); ++i)
        if (h->bufs[i].slot == reinterpret_cast<void**>(&h->sp_index)) { pool_free(h->sp_index, h->bufs[i].bytes, h->device, h->stream, true); h->bufs.erase(h->bufs.begin() + i); break; }
      h->sp_index = nullptr;
    }
    if ((rc = dalloc(h, &h->sp_index, arena.size(), false))) return rc;
    h->sp_index_ints = arena.size();
  }
  HIPCHK(hipMemcpyAsync(h->sp_index, arena.data(), arena.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
  h->sp_frame_off = h->sp_index + off[0]; h->sp_ent_cam = h->sp_index + off[1]; h->sp_ent_frame = h->sp_index + off[2]; h->sp_items = h->sp_index + off[3];
  h->sp_chunks = h->sp_index + off[4]; h->sp_pair_map = h->sp_index + off[5]; h->sp_pair_chunks = h->sp_index + off[6];
  // Y (72 doubles per entry) and the chunk sums (160 per chunk) grow with the index
  auto regrow = [&](double** p, size_t& have, size_t need) -> int {
    if (need <= have && *p) return MCBA_OK;
    if (*p) {
      for (size_t i = 0; i < h->bufs.size(); ++i)
        if (h->bufs[i].slot == reinterpret_cast<void**>(p)) { pool_free(*p, h->bufs[i].bytes, h->device, h->stream, true); h->bufs.erase(h->bufs.begin() + i); break; }
      *p = nullptr;
    }
    have = need;
    return dalloc(h, p, need, false);
  };
  if ((rc = regrow(&h->sp_Y, h->sp_Y_count, (size_t)72 * std::max(nent, 1)))) return rc;
  if ((rc = regrow(&h->sp_part, h->sp_part_count, (size_t)160 * std::max(nchunks, 1)))) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));   // (the host vectors above are pageable and about to go)
  h->sp_nent = nent;
  h->sp_npairs = npairs;
  h->sp_nchunks = nchunks;
  h->sp_ready = true;
  return MCBA_OK;
}

int sparse_build(mcba_handle* h, mcba::Sel sel) {
  int rc = sparse_index(h);
  if (rc) return rc;
  {
    Scope sc(h, K_SP_FACTOR);
    mcba::launch_sp_factor(h->stream, sel, h->rec2[0], h->rec2[1], h->fbuf, h->fpart, h->sp_frame_off, h->sp_ent_cam, h->sp_ent_frame, h->sp_nent, h->sp_Y, h->have_xscale ? h->dscale : nullptr,
                           h->C, h->F, h->Fpad, h->cw);
  }
  if ((rc = check_launch())) return rc;
  {
    Scope sc(h, K_SP_PAIRS);
    mcba::launch_sp_pairs(h->stream, sel, h->sp_Y, h->fbuf, h->sp_items, h->sp_chunks, h->sp_nchunks, h->sp_part, h->gpart2[0], h->gpart2[1], h->sp_pair_map, h->sp_pair_chunks, h->red, h->C,
                          h->nfb, h->cw);
  }
  return check_launch();
}

namespace {
struct SolveBracket {
  mcba_handle* h;
  Scope* open[5] = {};
};
void solve_bracket(void* ctx, int stage, int begin) {
  static const int kid[5] = {K_SP_SOLVE_PRE, K_SP_POTRF, K_SP_TRSM, K_SP_UPDATE, K_SP_FINISH};
  SolveBracket* b = static_cast<SolveBracket*>(ctx);
  if (!b->h->prof) return;
  if (begin) b->open[stage] = new Scope(b->h, kid[stage]);
  else { delete b->open[stage]; b->open[stage] = nullptr; }
}
}  // namespace

int sparse_solve(mcba_handle* h, const mcba::SolveArgs& a) {
  SolveBracket br{h};
  mcba::launch_sp_solve(h->stream, a, h->sp_ctl, h->sp_damp, h->sp_A, h->sp_y, solve_bracket, &br);
  return check_launch();
}

void sparse_forget(mcba_handle* h) {
  h->sp_ready = false;
  h->sp_index = h->sp_frame_off = h->sp_ent_cam = h->sp_ent_frame = h->sp_items = h->sp_chunks = h->sp_pair_map = h->sp_pair_chunks = nullptr;
  h->sp_ctl = nullptr;
  h->sp_Y = h->sp_part = h->sp_A = h->sp_damp = h->sp_y = nullptr;
  h->sp_index_ints = h->sp_Y_count = h->sp_part_count = 0;
}

}  // namespace mcba_internal

extern "C" {
// The visibility index of the sparse-Schur handle from a (C, F) mask, on the host (no device needed).  sizes: nent, npairs, nitems, nchunks.
// out (may be NULL = sizes only): frame_off (F + 1) | ent_cam (nent) | ent_frame (nent) | items (3 nitems: entry of camera i, entry of camera
// j, frame) | chunks (3 nchunks: first item, count, diagonal) | pair_map (C x C, pair id or -1) | pair_chunks (npairs + 1).
int mcba_sparse_index(const unsigned char* seen, int n_cameras, int n_frames, int* sizes, int* out, size_t capacity) {
  using namespace mcba_internal;
  if (!seen || !sizes || n_cameras < 1 || n_frames < 1) return fail(MCBA_ERR_ARG, "mcba_sparse_index: bad argument");
  SpIndex x;
  build_index(seen, n_cameras, n_frames, x);
  sizes[0] = (int)x.ent_cam.size(); sizes[1] = x.npairs; sizes[2] = (int)x.items.size() / 3; sizes[3] = (int)x.chunks.size() / 3;
  if (!out) return MCBA_OK;
  const size_t need = x.frame_off.size() + 2 * x.ent_cam.size() + x.items.size() + x.chunks.size() + x.pair_map.size() + x.pair_chunks.size();
  if (capacity < need) return fail(MCBA_ERR_ARG, "mcba_sparse_index: output too small");
  for (const std::vector<int>* v : {&x.frame_off, &x.ent_cam, &x.ent_frame, &x.items, &x.chunks, &x.pair_map, &x.pair_chunks}) {
    std::copy(v->begin(), v->end(), out);
    out += v->size();
  }
  return MCBA_OK;
}
}  // extern "C"
