// The decode host path: orchestration in C++, so that the per-token loop never returns to Python -- every decode step is one
// hipGraph replay; the host only polls a 4-byte "rows still running" word.  Chains and their stream pools, the cross-call cache of
// step graphs, the burst-and-poll launcher, mh_t5_generate* and the in-flight slot session mh_t5_slots_*.
// Host code only: this unit defines no kernel and launches none itself -- what a step enqueues, and every kernel launch around it,
// comes from t5_step.hip through decode_step.hpp (HF GenerationMixin._sample under model_generate, osuT5/osuT5/inference/server.py:83-156).
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "decode_step.hpp"
#include "t5_host.hpp"

using namespace mh;

namespace mh {
namespace {
// Independent rows => independent "chains": the batch is cut into contiguous blocks of rows and every
// block runs its own captured decode step on its own stream.  A decode step is ~110 dependent, mostly
// tiny kernels (each costs a few microseconds of dispatch + drain whatever its size), so one chain leaves
// the GPU idle most of the time; several chains overlap one another's dispatch gaps and let the
// HBM-bound cross-attention of one chain run under the latency-bound GEMVs of the others.  Results do not
// depend on the chain count (every kernel is batch-invariant by construction).
int pick_chains(int B) {
  int n = B >= 16 ? 2 : 1;   // measured on MI355X (B=32, base): 1 -> 26.7k, 2 -> 28.0k, 4 -> 17.6k tok/s (host graph-launch bound)
  if (option(OPT_DECODE_CHAINS) >= 1) n = (int)option(OPT_DECODE_CHAINS);
  if (n > kMaxChains) n = kMaxChains;
  if (n > B) n = B;
  return n;
}

struct ChainPool {   // extra streams + fork/join events of ONE device, created on first use under that device
  hipStream_t streams[kMaxChains] = {};
  hipEvent_t fork = nullptr, join[kMaxChains] = {};
  bool ready = false;
  int init() {
    if (ready) return MH_OK;
    if (hipEventCreateWithFlags(&fork, hipEventDisableTiming) != hipSuccess) return check_launch("event create");
    for (int i = 0; i < kMaxChains; ++i) {
      if (hipStreamCreateWithFlags(&streams[i], hipStreamNonBlocking) != hipSuccess ||
          hipEventCreateWithFlags(&join[i], hipEventDisableTiming) != hipSuccess)
        return check_launch("chain stream create");
    }
    ready = true;
    return MH_OK;
  }
};
// one pool per device; mh_t5_generate holds the pool's mutex for the whole call, so two engines (or two host
// threads) decoding on the same GPU take turns instead of sharing fork / join events
struct DevicePool { ChainPool pool; std::mutex mu; };
DevicePool* device_pool(int dev) {
  static std::mutex table_mu;
  static std::map<int, DevicePool*> table;
  std::lock_guard<std::mutex> g(table_mu);
  auto it = table.find(dev);
  if (it == table.end()) it = table.emplace(dev, new DevicePool()).first;
  return it->second;
}
}  // namespace
}  // namespace mh

extern "C" int64_t mh_t5_decode_workspace_bytes(const MhT5Config* c, int B) {
  mh::OptionScope option_scope(c ? c->options : nullptr);
  if (!c || B <= 0) return -1;
  return decode_layout(c, B, nullptr).end + prefill_layout(c, B, c->tgt_len - 1, nullptr, 0, nullptr);   // + batched prompt prefill
}

extern "C" int mh_t5_decode_self_cache(const MhT5Config* c, int B, void* workspace, void** k, void** v) {
  mh::OptionScope option_scope(c ? c->options : nullptr);
  MH_TRY(check_cfg(c, "mh_t5_decode_self_cache"));
  MH_REQUIRE(workspace && k && v && B > 0, "mh_t5_decode_self_cache: null argument");
  const mh::DecodeLayout ly = mh::decode_layout(c, B, workspace);
  *k = ly.bf.self_k;
  *v = ly.bf.self_v;
  return MH_OK;
}

namespace mh {
// ------------------------------------------------------------------------------------------------
// Instantiated step graphs kept ACROSS mh_t5_generate calls.  A chain's step graph bakes in nothing but addresses, sizes, the
// sampling struct and the kernel choice (the position and every per-call state live in device memory), so a later call
// whose inputs are byte-for-byte the same description -- the normal case of an engine that decodes window after window out
// of the same workspace with the same prompt length -- replays the graph of the earlier one instead of capturing and
// instantiating ~75 nodes again.  The key comes from ONE place: step_graph_key() over the StepCall that enqueue_step() is given,
// the only thing it reads besides the options -- so whatever a step depends on is in its key (exact compare: a spurious
// difference costs a capture, never a wrong graph).  Small LRU; an entry in use by a concurrent call is never shared
// (hipGraphExec objects are single-flight) nor evicted.  Option decode_graph_cache = 0 switches it off.
struct StepGraphEntry {
  std::vector<unsigned char> key;      // step_graph_key(StepCall)
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  uint64_t stamp = 0;
  bool in_use = false;
};
constexpr size_t kStepGraphCacheMax = 16;
static std::mutex g_step_graph_mu;
static std::vector<StepGraphEntry*> g_step_graphs;
static uint64_t g_step_graph_clock = 0;
static std::atomic<long> g_step_graph_hits{0}, g_step_graph_misses{0};

// The bytes of the StepCall, then what it depends on beyond them: *c without the address of its option set, *w, every option value,
// the device, the storage type.  Scrubbed, here and nowhere else: the addresses of c and w (their contents follow); seed and rng_row0
// (they reach the sampler through DecState, not through the graph); under the row form what that sampler reads per row instead.
static std::vector<unsigned char> step_graph_key(const StepCall& call) {
  std::vector<unsigned char> key;
  auto put = [&key](const void* p, size_t n) { key.insert(key.end(), (const unsigned char*)p, (const unsigned char*)p + n); };
  StepCall k;
  memcpy(&k, &call, sizeof(k));
  k.c = nullptr; k.w = nullptr;
  MhSampling& sp = k.smp.sp;
  sp.seed = 0; sp.rng_row0 = 0;
  if (k.has_rows) {
    k.smp.eos_table = nullptr;
    sp.cfg_scale = sp.cfg_scale > 1.0f ? 2.f : 1.f;   // (guidance on / off is the call's, the scale each pair's own)
    sp.temperature = sp.top_p = sp.timeshift_bias = 0.f;
    sp.top_k = sp.lookback_mask_end = 0;
    for (int j = 0; j < 3; ++j) sp.cond_temp[j] = 0.f;
  }
  MhT5Config cc = *call.c;
  cc.options = nullptr;
  long opts[OPT_COUNT];
  for (int o = 0; o < OPT_COUNT; ++o) opts[o] = option(o);
  int dev_id = 0;
  (void)hipGetDevice(&dev_id);
  const int ids[2] = {dev_id, call.c->dtype == MH_BF16 ? 1 : 0};
  put(&k, sizeof(k)); put(&cc, sizeof(cc)); put(call.w, sizeof(*call.w)); put(opts, sizeof(opts)); put(ids, sizeof(ids));
  return key;
}

static StepGraphEntry* step_graph_acquire(const std::vector<unsigned char>& key) {
  std::lock_guard<std::mutex> lk(g_step_graph_mu);
  for (StepGraphEntry* e : g_step_graphs)
    if (!e->in_use && e->key == key) {
      e->in_use = true;
      e->stamp = ++g_step_graph_clock;
      return e;
    }
  return nullptr;
}

// takes ownership of graph / exec; returns the entry (in use) -- or nullptr when the cache is full of entries in use
static StepGraphEntry* step_graph_insert(std::vector<unsigned char>&& key, hipGraph_t graph, hipGraphExec_t exec) {
  std::lock_guard<std::mutex> lk(g_step_graph_mu);
  while (g_step_graphs.size() >= kStepGraphCacheMax) {
    int victim = -1;
    for (size_t i = 0; i < g_step_graphs.size(); ++i)
      if (!g_step_graphs[i]->in_use && (victim < 0 || g_step_graphs[i]->stamp < g_step_graphs[victim]->stamp)) victim = (int)i;
    if (victim < 0) return nullptr;
    StepGraphEntry* v = g_step_graphs[victim];
    (void)hipGraphExecDestroy(v->exec);
    (void)hipGraphDestroy(v->graph);
    delete v;
    g_step_graphs.erase(g_step_graphs.begin() + victim);
  }
  StepGraphEntry* e = new StepGraphEntry();
  e->key = std::move(key);
  e->graph = graph;
  e->exec = exec;
  e->in_use = true;
  e->stamp = ++g_step_graph_clock;
  g_step_graphs.push_back(e);
  return e;
}

static void step_graph_release(StepGraphEntry* e) {
  std::lock_guard<std::mutex> lk(g_step_graph_mu);
  e->in_use = false;
}

// The device that owns the caller's stream (not whatever happens to be current)
static int stream_device(hipStream_t s, int* dev) {
  if (hipStreamGetDevice(s, dev) != hipSuccess) { (void)hipGetLastError(); if (hipGetDevice(dev) != hipSuccess) return check_launch("hipGetDevice"); }
  return MH_OK;
}
// Streams, events and graphs of a call or a session are created under that device; the current one is restored on every return path
struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int want) { if (hipGetDevice(&prev) == hipSuccess && prev != want) (void)hipSetDevice(want); else prev = -1; }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// A chain of the running call and the owner of its step graph: the cross-call cache (`cached`: handed back when the call ends) or the
// call itself (destroyed with it, after the call's last synchronise)
struct Chain {
  hipStream_t stream = nullptr; DecState* st = nullptr;
  hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr; StepGraphEntry* cached = nullptr;
  Chain() = default;
  Chain(const Chain&) = delete;
  Chain& operator=(const Chain&) = delete;
  ~Chain() {
    if (cached) { step_graph_release(cached); return; }
    if (exec) (void)hipGraphExecDestroy(exec);
    if (graph) (void)hipGraphDestroy(graph);
  }
};

// A chain enters the call on its own stream, behind the caller's work so far (`fork`): dec_init_kernel, then one step of the chain (every
// kernel reads the position from device memory) as a graph for replay: an earlier call's, if its key is this one's, else captured now
static int chain_step_graph(const StepCall& call, const char* who, Chain* ch);
static int start_chain(const StepCall& call, int start_pos, hipEvent_t fork, const char* who, Chain* ch) {
  hipStream_t cs = ch->stream;
  ch->st = call.bf.st;
  if (hipStreamWaitEvent(cs, fork, 0) != hipSuccess) return check_launch("fork wait");
  MH_TRY(launch_dec_init(call.c->dtype, call.smp, call.Bc, start_pos, cs));
  return chain_step_graph(call, who, ch);
}
// One step of the chain as a graph for replay on ch->stream: an earlier call's, if its key is this one's, else captured now
static int chain_step_graph(const StepCall& call, const char* who, Chain* ch) {
  hipStream_t cs = ch->stream;
  std::vector<unsigned char> key;
  if (option(OPT_DECODE_GRAPH_CACHE) != 0) {
    key = step_graph_key(call);
    if ((ch->cached = step_graph_acquire(key))) { ch->exec = ch->cached->exec; g_step_graph_hits.fetch_add(1); return MH_OK; }
    g_step_graph_misses.fetch_add(1);
  }
  if (hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal) != hipSuccess) return check_launch("begin capture");
  const int rce = enqueue_step(call, cs);
  const hipError_t ce = hipStreamEndCapture(cs, &ch->graph);
  if (rce != MH_OK) return rce;
  if (ce != hipSuccess || !ch->graph) { set_error("%s: stream capture failed: %s", who, hipGetErrorString(ce)); return MH_ERR_LAUNCH; }
  if (hipGraphInstantiate(&ch->exec, ch->graph, nullptr, nullptr, 0) != hipSuccess) return check_launch("graph instantiate");
  if (!key.empty() && (ch->cached = step_graph_insert(std::move(key), ch->graph, ch->exec))) ch->graph = nullptr;   // the cache owns both now
  return MH_OK;
}

// The host's look at a chain between two bursts of replays: DecState::n_running and ::tail_err in one 8-byte read
static int poll_chain(const Chain& ch, bool* running) {
  int word[2] = {1, 0};
  if (hipMemcpyAsync(word, &ch.st->n_running, 8, hipMemcpyDeviceToHost, ch.stream) != hipSuccess ||
      hipStreamSynchronize(ch.stream) != hipSuccess)
    return MH_ERR_LAUNCH;
  *running = word[0] != 0;
  return word[1] != 0 ? MH_ERR_DECODE_TAIL_TIMEOUT : MH_OK;
}

// The one burst-and-poll loop, of a uniform call and of a slot session alike.  The launcher of chains which[0 .. n) from the calling
// thread: bursts of poll_every replays each, interleaved, then a poll of each (none behind the last burst, none under teacher forcing:
// poll = false).  A chain is left out once its rows are done or it failed (rcs[chain]); replays[chain], if given, counts its
// hipGraphLaunch calls that succeeded.
static void run_chains(const Chain* chains, const int* which, int n, int n_steps, int poll_every, bool poll, int* rcs, int* replays) {
  bool alive[kMaxChains];
  for (int i = 0; i < n; ++i) alive[i] = true;
  for (int step = 0; step < n_steps;) {
    const int burst = n_steps - step < poll_every ? n_steps - step : poll_every;
    for (int r = 0; r < burst; ++r)
      for (int i = 0; i < n; ++i) {
        const int ci = which[i];
        if (!alive[i] || rcs[ci] != MH_OK) continue;
        if (hipGraphLaunch(chains[ci].exec, chains[ci].stream) != hipSuccess) rcs[ci] = MH_ERR_LAUNCH;
        else if (replays) ++replays[ci];
      }
    step += burst;
    bool any = false;
    for (int i = 0; i < n; ++i) {
      const int ci = which[i];
      if (!alive[i] || rcs[ci] != MH_OK) continue;
      if (step < n_steps && poll && (rcs[ci] = poll_chain(chains[ci], &alive[i])) != MH_OK) continue;
      any = any || alive[i];
    }
    if (!any) break;
  }
}
// Replaying a ~110-node graph costs ~0.4 ms of HOST time on ROCm 7.2, so every running chain gets a launcher thread of its own (the
// chains are independent; the first runs on the calling thread); option decode_launch_threads = 0: one launcher for all, their bursts
// interleaved (slower on the host side; the same kernels and arguments).  which: the chains that run -- all of a uniform call, those
// with a live slot of a session.  -> the call's status, the failed chain named by its index
static int launch_chains(const Chain* chains, const int* which, int n, int n_steps, int poll_every, bool poll, const char* who,
                         int* replays = nullptr) {
  int rcs[kMaxChains] = {};
  if (n <= 1 || option(OPT_DECODE_LAUNCH_THREADS) == 0) {
    run_chains(chains, which, n, n_steps, poll_every, poll, rcs, replays);
  } else {
    std::vector<std::thread> th;
    const MhOptionSet* set = current_option_set();   // thread-local in the caller: re-installed in every launcher
    for (int i = 1; i < n; ++i)
      th.emplace_back([&, i, set] { OptionScope sc(set); run_chains(chains, which + i, 1, n_steps, poll_every, poll, rcs, replays); });
    run_chains(chains, which, 1, n_steps, poll_every, poll, rcs, replays);
    for (auto& t : th) t.join();
  }
  int rc = MH_OK;
  for (int i = 0; i < n; ++i) {
    const int ci = which[i];
    if (rcs[ci] == MH_ERR_DECODE_TAIL_TIMEOUT) rc = mh_t5_decode_tail_status(1);
    else if (rcs[ci] != MH_OK) { set_error("%s: graph launch / poll failed on chain %d: %s", who, ci, hipGetErrorString(hipGetLastError())); rc = rcs[ci]; }
  }
  return rc;
}

// What mh_t5_generate, mh_t5_generate_skv8 (self_kv_fp8: the caller's e4m3 shadow of the self-attention cache, else NULL) and
// mh_t5_generate_rows (rowset: the sampler's settings per returned row, else NULL) were given; who: the entry, for error messages
struct GenerateArgs {
  const MhT5Config* c; const MhT5Weights* w; const void* cross_kv; int B; const int32_t* prompt; const uint8_t* prompt_mask; int P;
  const uint8_t* eos_table; const MhSampling* sp; int32_t* tokens; int32_t* n_steps_out; float* logits_dump; const int32_t* forced;
  void* workspace; int64_t workspace_bytes; int poll_every; void* stream; void* self_kv_fp8; const RowSetP* rowset; const char* who;
};

// What every entry that runs the sampled token step checks of its configuration and settings, in this order (ptrs_ok: the entry's own
// pointer arguments are all there; P: the call's prompt length, or NULL where every row brings its own -- mh_t5_slots_admit checks it)
static int check_decode_call(const MhT5Config* c, const MhT5Weights* w, const MhSampling* sp, int B, bool ptrs_ok, void* stream,
                             const int* P, bool rows, const char* who) {
  MH_TRY(check_cfg(c, who));
  MH_TRY(check_decode_shape(c, who));
  MH_REQUIRE(w && sp && ptrs_ok, "%s: null argument", who);
  MH_REQUIRE(stream != nullptr, "%s: needs a non-default stream (hipGraph capture)", who);
  MH_REQUIRE(B > 0 && B <= 64, "%s: batch %d not in [1, 64] (shard larger batches on the host)", who, B);
  MH_REQUIRE(!P || (*P >= 1 && *P < sp->max_length), "%s: prompt length %d must be in [1, max_length)", who, P ? *P : 0);
  MH_REQUIRE(sp->max_length >= 2, "%s: max_length %d must be >= 2", who, sp->max_length);
  MH_REQUIRE(sp->max_length <= c->tgt_len, "%s: max_length %d exceeds tgt_len %d", who, sp->max_length, c->tgt_len);
  MH_REQUIRE(rows || sp->temperature > 0.f, "%s: temperature must be > 0", who);
  MH_REQUIRE(sp->n_sos >= 0 && sp->n_sos <= 16, "%s: too many sos ids", who);
  MH_REQUIRE(!(sp->cfg_scale > 1.0f) || B % 2 == 0, "%s: classifier-free guidance needs an even batch (negative rows, then prompt rows)", who);
  MH_REQUIRE(sp->n_cond >= 0 && sp->n_cond <= 3, "%s: n_cond %d not in [0, 3]", who, sp->n_cond);
  for (int j = 0; j < sp->n_cond; ++j)
    MH_REQUIRE((rows || sp->cond_temp[j] > 0.f) && sp->cond_offset[j] >= 1, "%s: bad conditional temperature rule %d", who, j);
  MH_REQUIRE(sp->tok_flags || (sp->n_cond == 0 && !sp->lookback_types_first),
             "%s: tok_flags is required by the conditional temperature / types_first lookback processors", who);
  MH_REQUIRE(!sp->cross_kv_fp8 || c->dtype == MH_BF16, "%s: cross_kv_fp8 needs bf16 storage", who);
  return MH_OK;
}

// The row settings of mh_t5_generate_rows (one entry per: "returned row") and of mh_t5_slots_open ("slot")
static int check_row_set(const MhRowSampling* rows, const uint8_t* eos_tables, int n_eos_sets, const char* per, const char* who) {
  MH_REQUIRE(rows && eos_tables, "%s: null argument (rows: one MhRowSampling per %s; eos_tables: [n_eos_sets][vocab_out])", who, per);
  MH_REQUIRE(n_eos_sets >= 1, "%s: n_eos_sets %d must be >= 1", who, n_eos_sets);
  return MH_OK;
}

static int check_generate_args(const GenerateArgs& a) {
  const bool ptrs_ok = a.cross_kv && a.prompt && (a.eos_table || a.rowset) && a.tokens && a.n_steps_out && a.workspace;
  MH_TRY(check_decode_call(a.c, a.w, a.sp, a.B, ptrs_ok, a.stream, &a.P, a.rowset != nullptr, a.who));
  MH_REQUIRE(a.workspace_bytes >= mh_t5_decode_workspace_bytes(a.c, a.B), "%s: workspace too small", a.who);
  return check_arch2_weights(a.c, a.w, a.who);
}

// Chain ci of the call as a StepCall: rows [ci rows_per, + Bc) of every buffer, of the e4m3 copies and of the sampler's view
// (Bc <= 0: the batch has no such chain).  self8: the shadow of the whole batch, or NULL.
static void chain_call(const GenerateArgs& a, const DecodeLayout& ly, int ci, int rows_per, uint8_t* self8, StepCall* k) {
  const MhT5Config* c = a.c;
  const MhSampling* sp = a.sp;
  const DecBuffers& all = ly.bf;
  const int B = a.B, P = a.P, es = es_of(c->dtype), H = c->n_heads, inner = H * 64, d = c->d_model, V = c->vocab_out;
  const bool cfg = sp->cfg_scale > 1.0f;
  const int b0 = ci * rows_per;
  step_call_init(k, c, a.w);
  k->Bc = (b0 + rows_per <= B) ? rows_per : B - b0;
  k->Bfull = B; k->kvB = cfg ? B / 2 : B; k->P = P; k->with_sampler = 1;
  k->cross_kv = a.cross_kv ? (const char*)a.cross_kv + (long)b0 * H * c->src_len * 64 * es : nullptr;   // (NULL: a kv8 slot session without one)
  k->prompt_mask = a.prompt_mask ? a.prompt_mask + (long)b0 * P : nullptr;
  if (a.rowset) { k->has_rows = 1; k->rows.rows = a.rowset->rows; k->rows.eos_tables = a.rowset->eos_tables; k->rows.n_eos_sets = a.rowset->n_eos_sets; }
  DecBuffers& bf = k->bf;
  bf.chain = ci;
  bf.h = all.h + (long)b0 * d;
  bf.attn = (char*)all.attn + (long)b0 * inner * es;
  bf.ff = (char*)all.ff + (long)b0 * c->d_ff * es;
  bf.logits = all.logits + (long)b0 * V;
  bf.self_k = (char*)all.self_k + (long)b0 * inner * c->tgt_len * es;
  bf.self_v = (char*)all.self_v + (long)b0 * inner * c->tgt_len * es;
  if (self8) self8_rows(c, B, b0, self8, &bf);
  bf.finished = all.finished + b0;
  bf.finish_col = all.finish_col; bf.last_ts = all.last_ts;
  bf.st = (DecState*)((char*)all.st + (long)ci * align256(sizeof(DecState)));
  if (sp->cross_kv_fp8) cross8_rows(c, k->kvB, b0, sp->cross_kv_fp8, k);
  SampleP& smp = k->smp;
  smp.logits = bf.logits; smp.ldl = V; smp.V = V; smp.tokens = a.tokens; smp.max_length = sp->max_length;
  smp.forced = a.forced; smp.eos_table = a.eos_table; smp.finished = all.finished; smp.finish_col = all.finish_col;
  smp.last_ts_val = all.last_ts; smp.logits_dump = a.logits_dump; smp.dec_embed = a.w->dec_embed; smp.h = bf.h;
  smp.d = d; smp.st = bf.st; smp.B = B; smp.P = P; smp.b0 = b0;
  memcpy(&smp.sp, sp, sizeof(*sp));
  smp.proc = ly.proc; smp.hist_scores = ly.hist_scores; smp.pair = cfg ? B / 2 : 0; smp.chain_rows = k->Bc;
  if (c->arch == 2) {
    smp.dec_pos = a.w->dec_pos;
    smp.pos_off = c->dec_pos_from_mask ? ly.pos_off : nullptr;
    smp.prompt_mask = a.prompt_mask;
  }
}
// The batch cut into n_chains blocks of rows_per rows: calls[0 .. used), -> used (a late block may be empty: B = 5 over 4 chains)
static int chain_calls(const GenerateArgs& a, const DecodeLayout& ly, int n_chains, int rows_per, uint8_t* self8, StepCall* calls) {
  int used = 0;
  for (; used < n_chains; ++used) {
    chain_call(a, ly, used, rows_per, self8, &calls[used]);
    if (calls[used].Bc <= 0) break;
  }
  return used;
}

static int generate_impl(const GenerateArgs& a) {
  MH_TRY(check_generate_args(a));
  const MhT5Config* c = a.c;
  const MhSampling* sp = a.sp;
  const int B = a.B, P = a.P;
  hipStream_t s = (hipStream_t)a.stream;
  const bool cfg = sp->cfg_scale > 1.0f;
  const DecodeLayout ly = decode_layout(c, B, a.workspace);
  // a CFG pair spans both halves of the batch and the (batch-wide) conditional temperature reads row 0's history: one chain
  const int n_chains = (cfg || (sp->n_cond > 0 && !sp->cond_per_row)) ? 1 : pick_chains(B);
  const int rows_per = ceil_div(B, n_chains);
  int dev = 0;
  MH_TRY(stream_device(s, &dev));
  DeviceGuard device_guard(dev);
  DevicePool* dp = device_pool(dev);
  std::lock_guard<std::mutex> pool_guard(dp->mu);
  ChainPool& g_pool = dp->pool;
  MH_TRY(g_pool.init());
  Chain chains[kMaxChains];   // (their graphs are released / destroyed on every return path below)
  for (int i = 0; i < kMaxChains; ++i) chains[i].stream = g_pool.streams[i];

  // tokens[:, :P] = prompt; the remainder is produced by the sampler
  if (hipMemcpy2DAsync(a.tokens, (size_t)sp->max_length * 4, a.prompt, (size_t)P * 4, (size_t)P * 4, B,
                       hipMemcpyDeviceToDevice, s) != hipSuccess)
    return check_launch("prompt copy");
  // batched prompt prefill (positions 0..P-2); MH_DECODE_PREFILL=0 feeds the prompt token by token instead
  int start_pos = 0;
  if (P > 1 && option(OPT_DECODE_PREFILL) != 0) {
    PrefillBuf pb;
    prefill_layout(c, B, P - 1, (char*)a.workspace + ly.end, a.workspace_bytes - ly.end, &pb);
    MH_REQUIRE(ly.end + prefill_layout(c, B, P - 1, nullptr, 0, nullptr) <= a.workspace_bytes,
               "%s: workspace too small for the prompt prefill", a.who);
    MH_TRY(prefill_prompt(c, a.w, a.cross_kv, B, cfg ? B / 2 : B, a.prompt, a.prompt_mask, P, P - 1, ly.bf.self_k, ly.bf.self_v, pb, s));
    start_pos = P - 1;
  }
  // the shadow: the prompt positions the batched prefill wrote (they attended each other through the bf16 cache) are quantised in
  // one pass before the first token step; every token step appends its own row
  uint8_t* self8 = (uint8_t*)a.self_kv_fp8;
  if (self8 && start_pos > 0) MH_TRY(launch_self_kv_quant_rows(c, B, ly.bf, self8, B, start_pos, s));
  if (hipEventRecord(g_pool.fork, s) != hipSuccess) return check_launch("fork record");

  StepCall calls[kMaxChains];
  const int used = chain_calls(a, ly, n_chains, rows_per, self8, calls);
  int rc = MH_OK, which[kMaxChains];   // every chain of the call runs
  for (int ci = 0; ci < used && rc == MH_OK; ++ci) {
    which[ci] = ci;
    rc = start_chain(calls[ci], start_pos, g_pool.fork, a.who, &chains[ci]);
  }

  const int total_steps = sp->max_length - 1 - start_pos;   // positions start_pos .. max_length-2 are fed
  if (rc == MH_OK) rc = launch_chains(chains, which, used, total_steps, a.poll_every <= 0 ? 16 : a.poll_every, !a.forced, a.who);
  // join the chains back into the caller's stream
  for (int ci = 0; ci < used; ++ci) {
    (void)hipEventRecord(g_pool.join[ci], chains[ci].stream);
    (void)hipStreamWaitEvent(s, g_pool.join[ci], 0);
  }
  if (rc == MH_OK) rc = launch_dec_finalize(ly.bf.finish_col, B, a.n_steps_out, s);
  (void)hipStreamSynchronize(s);   // the graph objects must outlive their launches
  if (rc == MH_OK && option(OPT_DECODE_FUSED_TAIL) != 0) {   // the chains are idle: their last word on the bounded hand-offs
    for (int ci = 0; ci < used && rc == MH_OK; ++ci) {
      int err = 0;
      if (hipMemcpy(&err, &chains[ci].st->tail_err, 4, hipMemcpyDeviceToHost) != hipSuccess) rc = check_launch("tail status");
      else rc = mh_t5_decode_tail_status(err);
    }
  }
  return rc;
}
}  // namespace mh

extern "C" int mh_t5_step_graph_cache_stats(long* hits, long* misses, int reset) {
  if (hits) *hits = mh::g_step_graph_hits.load();
  if (misses) *misses = mh::g_step_graph_misses.load();
  if (reset) { mh::g_step_graph_hits.store(0); mh::g_step_graph_misses.store(0); }
  return MH_OK;
}

extern "C" int mh_t5_generate(const MhT5Config* c, const MhT5Weights* w, const void* cross_kv, int B,
                              const int32_t* prompt, const uint8_t* prompt_mask, int P, const uint8_t* eos_table,
                              const MhSampling* sp, int32_t* tokens, int32_t* n_steps_out, float* logits_dump,
                              const int32_t* forced, void* workspace, int64_t workspace_bytes, int poll_every,
                              void* stream) {
  mh::OptionScope option_scope(c ? c->options : nullptr);
  return generate_impl({c, w, cross_kv, B, prompt, prompt_mask, P, eos_table, sp, tokens, n_steps_out, logits_dump, forced, workspace,
                        workspace_bytes, poll_every, stream, nullptr, nullptr, "mh_t5_generate"});
}

extern "C" int mh_t5_generate_skv8(const MhT5Config* c, const MhT5Weights* w, const void* cross_kv, int B,
                                   const int32_t* prompt, const uint8_t* prompt_mask, int P, const uint8_t* eos_table,
                                   const MhSampling* sp, int32_t* tokens, int32_t* n_steps_out, float* logits_dump,
                                   const int32_t* forced, void* workspace, int64_t workspace_bytes, int poll_every,
                                   void* stream, void* self_kv_fp8) {
  mh::OptionScope option_scope(c ? c->options : nullptr);
  MH_TRY(check_cfg(c, "mh_t5_generate_skv8"));
  MH_REQUIRE(self_kv_fp8, "mh_t5_generate_skv8: null argument (self_kv_fp8: mh_t5_self_kv_fp8_bytes(cfg, B) bytes owned by the caller)");
  MH_REQUIRE(c->dtype == MH_BF16, "mh_t5_generate_skv8: the e4m3 self-attention cache needs bf16 storage");
  return generate_impl({c, w, cross_kv, B, prompt, prompt_mask, P, eos_table, sp, tokens, n_steps_out, logits_dump, forced, workspace,
                        workspace_bytes, poll_every, stream, self_kv_fp8, nullptr, "mh_t5_generate_skv8"});
}

extern "C" int mh_t5_generate_rows(const MhT5Config* c, const MhT5Weights* w, const void* cross_kv, int B,
                                   const int32_t* prompt, const uint8_t* prompt_mask, int P, const uint8_t* eos_table,
                                   const MhSampling* sp, int32_t* tokens, int32_t* n_steps_out, float* logits_dump,
                                   const int32_t* forced, void* workspace, int64_t workspace_bytes, int poll_every,
                                   void* stream, void* self_kv_fp8, const MhRowSampling* rows, const uint8_t* eos_tables,
                                   int n_eos_sets) {
  mh::OptionScope option_scope(c ? c->options : nullptr);
  (void)eos_table;   // ignored: every row names its set of eos_tables
  MH_TRY(check_cfg(c, "mh_t5_generate_rows"));
  MH_TRY(mh::check_row_set(rows, eos_tables, n_eos_sets, "returned row", "mh_t5_generate_rows"));
  MH_REQUIRE(!self_kv_fp8 || c->dtype == MH_BF16, "mh_t5_generate_rows: the e4m3 self-attention cache needs bf16 storage");
  const mh::RowSetP rowset{rows, eos_tables, n_eos_sets};
  return generate_impl({c, w, cross_kv, B, prompt, prompt_mask, P, nullptr, sp, tokens, n_steps_out, logits_dump, forced, workspace,
                        workspace_bytes, poll_every, stream, self_kv_fp8, &rowset, "mh_t5_generate_rows"});
}

// ------------------------------------------------------------------------------------------------
// In-flight decode (mh_t5_slots_*; contract in include/mapperhip.h): S slots, every slot a row with a window of its own that enters
// (admit) and leaves (release) while its neighbours keep stepping.  The chains are those of mh_t5_generate_rows over S rows -- the
// same static row blocks, one DecState and one step graph each (the SLOT kernels: the key holds StepCall::slot_pos) -- on streams
// the session owns; admissions run on a stream of their own.
//
// Why no step can write a cache row, a token or a state word that an admission is filling, and no admission one that a step reads:
//   * an idle slot's position is negative: its self-attention workgroups return before they store, its sampler workgroup only
//     arrives; the GEMVs, the tail and the cross-attention write the slot's rows of h / attn / ff / logits, which nothing reads;
//   * release(slot) makes the position negative ON THE CHAIN'S STREAM, behind the slot's last step, and records freed[slot] there;
//   * admit(slot) waits for freed[slot] on the admission stream before its first write, and the slot's position -- the one word that
//     makes it live -- is the last thing its last kernel writes; then it records admitted[chain];
//   * run() makes the chain's stream wait for admitted[chain] before the first step enqueued after the admission.
// Events only: nothing on the device spins or waits for another launch.
//
// A guided session (mh_t5_slots_open_guided): every slot is a classifier-free guidance PAIR, decode rows s (negative prompt) and S + s
// (prompt) of R = 2 S rows -- the row order of a guided mh_t5_generate_rows call, so the token step is that call's (kvB = S, pair =
// S, one chain) with the sampler in its PAIR form.  Every array below that is "per row" has R entries and both rows of a pair always
// hold the same position; live / freed / the host's view are per slot.  Admission, release and the poll treat the two rows as one.
namespace mh {
struct SlotSession {
  const MhT5Config* c = nullptr; const MhT5Weights* w = nullptr;
  int S = 0, n_chains = 0, rows_per = 0, dev = 0, max_length = 0, poll_every = 16;
  int R = 0; bool guided = false;   // R: decode rows, S or (guided) 2 S
  DecodeLayout ly{};
  int32_t* pos = nullptr; int32_t* plen = nullptr; uint8_t* mask = nullptr;   // [R], [R], [R][max_length]
  char* prefill_base = nullptr; int64_t prefill_bytes = 0;
  char* cross_kv = nullptr; int32_t* tokens = nullptr;   // cross_kv: the bf16 / fp32 slot copy, NULL where the steps stream cross8 alone
  uint8_t* cross8 = nullptr; uint8_t* self8 = nullptr;   // mh_t5_slots_open_kv8: the caller's S-row e4m3 copies, or NULL
  Chain chains[kMaxChains];
  StepCall calls[kMaxChains];
  hipStream_t admit_stream = nullptr;
  hipEvent_t admitted[kMaxChains] = {}, freed[64] = {}, caller_ev = nullptr;
  bool pending[kMaxChains] = {};    // an admission into the chain since its last step was enqueued
  bool live[64] = {};               // admitted and not released
  int32_t host_pos[64] = {}, host_col[64] = {}; uint8_t host_fin[64] = {};
  ~SlotSession() {
    // joins the chains and the admissions (a graph object must outlive its launches; the Chain members release theirs after this body)
    if (admit_stream) { (void)hipStreamSynchronize(admit_stream); (void)hipStreamDestroy(admit_stream); }
    for (int i = 0; i < kMaxChains; ++i) {
      if (chains[i].stream) { (void)hipStreamSynchronize(chains[i].stream); (void)hipStreamDestroy(chains[i].stream); }
      if (admitted[i]) (void)hipEventDestroy(admitted[i]);
    }
    for (int i = 0; i < 64; ++i) if (freed[i]) (void)hipEventDestroy(freed[i]);
    if (caller_ev) (void)hipEventDestroy(caller_ev);
  }
  int chain_of(int slot) const { return slot / rows_per; }
  int row_of(int slot) const { return guided ? S + slot : slot; }   // the row whose ids are the window's (the prompt row of a pair)
};
// the slot buffers behind the decode layout of R rows (S, or 2 S of a guided session), then the prompt prefill of ONE window (a row,
// or the two rows of a pair)
static int64_t slots_layout(const MhT5Config* c, int S, void* base, SlotSession* ss, bool guided = false) {
  const int R = guided ? 2 * S : S;
  const DecodeLayout ly = decode_layout(c, R, base);
  Arena ar(base ? (char*)base + ly.end : nullptr, INT64_MAX);
  int32_t* pos = (int32_t*)ar.take((int64_t)R * 4);
  int32_t* plen = (int32_t*)ar.take((int64_t)R * 4);
  uint8_t* mask = (uint8_t*)ar.take((int64_t)R * c->tgt_len);
  const int64_t pre = prefill_layout(c, guided ? 2 : 1, c->tgt_len - 1, nullptr, 0, nullptr);
  if (ss) {
    ss->ly = ly; ss->pos = pos; ss->plen = plen; ss->mask = mask;
    ss->prefill_base = (char*)base + ly.end + ar.off; ss->prefill_bytes = pre;
  }
  return ly.end + ar.off + pre;
}
}  // namespace mh

extern "C" int64_t mh_t5_slots_workspace_bytes(const MhT5Config* c, int S) {
  mh::OptionScope option_scope(c ? c->options : nullptr);
  if (!c || S < 1 || S > 64) return -1;
  return mh::slots_layout(c, S, nullptr, nullptr);
}

extern "C" int64_t mh_t5_slots_guided_workspace_bytes(const MhT5Config* c, int S) {
  mh::OptionScope option_scope(c ? c->options : nullptr);
  if (!c || S < 1 || S > 32) return -1;   // a decode batch holds 64 rows
  return mh::slots_layout(c, S, nullptr, nullptr, true);
}

namespace mh {
// mh_t5_slots_open (kv8 = false: the e4m3 caches are refused) and mh_t5_slots_open_kv8 (kv8 = true: sp->cross_kv_fp8 / self_kv_fp8 are
// the session's S-row copies, filled row by row by the admissions and the token steps); guided: mh_t5_slots_open_guided, S pairs over
// 2 S decode rows on one chain (a pair spans both halves of the batch, as in generate_impl), the shadow of 2 S rows, the cross copies
// of S
static int slots_open_impl(const MhT5Config* c, const MhT5Weights* w, int S, const MhSampling* sp, const MhRowSampling* rows,
                           const uint8_t* eos_tables, int n_eos_sets, void* cross_kv_slots, int32_t* tokens, float* logits_dump,
                           const int32_t* forced, void* self_kv_fp8, void* workspace, int64_t workspace_bytes, int poll_every,
                           void* stream, void** handle, bool kv8, const char* who, bool guided = false) {
  OptionScope option_scope(c ? c->options : nullptr);
  MH_TRY(check_cfg(c, who));
  MH_REQUIRE(handle, "%s: null argument (handle)", who);
  *handle = nullptr;
  if (guided) MH_REQUIRE(S >= 1 && S <= 32, "%s: %d pairs not in [1, 32] (a decode batch holds 64 rows)", who, S);
  else MH_REQUIRE(S >= 1 && S <= 64, "%s: %d slots not in [1, 64]", who, S);
  const int R = guided ? 2 * S : S;
  MH_TRY(check_row_set(rows, eos_tables, n_eos_sets, guided ? "pair" : "slot", who));
  MH_REQUIRE(sp, "%s: null argument (sp)", who);
  if (guided) MH_REQUIRE(sp->cfg_scale > 1.0f, "%s: needs sp->cfg_scale > 1 (every slot is a guidance pair; the scale is each pair's own, rows[slot].cfg_scale)", who);
  else MH_REQUIRE(!(sp->cfg_scale > 1.0f), "%s: classifier-free guidance has no slot form (a pair spans two rows of one position)", who);
  MH_REQUIRE(!forced, "%s: teacher forcing (forced ids) has no slot form", who);
  if (!kv8) {
    MH_REQUIRE(!sp->cross_kv_fp8, "%s: the e4m3 copy of the cross K/V (cross_kv_fp8) has no slot form", who);
    MH_REQUIRE(!self_kv_fp8, "%s: the e4m3 shadow of the self-attention cache has no slot form", who);
  } else {
    MH_REQUIRE(!sp->cross_kv_fp8 || c->dtype == MH_BF16, "%s: cross_kv_fp8 needs bf16 storage", who);
    MH_REQUIRE(!self_kv_fp8 || c->dtype == MH_BF16, "%s: the e4m3 self-attention cache needs bf16 storage", who);
    MH_REQUIRE(cross_kv_slots || sp->cross_kv_fp8,
               "%s: null argument (cross_kv_slots may be NULL only where sp->cross_kv_fp8 is the slots' e4m3 copy)", who);
  }
  MH_REQUIRE(sp->n_cond == 0 || sp->cond_per_row, "%s: conditional temperature rules need cond_per_row = 1 (every slot is a window of its own)", who);
  // whatever mh_t5_generate_rows refuses of a configuration and its settings (the prompt length is each admission's)
  MH_TRY(check_decode_call(c, w, sp, R, (cross_kv_slots || (kv8 && sp->cross_kv_fp8)) && tokens && workspace, stream, nullptr, true, who));
  MH_REQUIRE(workspace_bytes >= slots_layout(c, S, nullptr, nullptr, guided), "%s: workspace too small (%s)", who,
             guided ? "mh_t5_slots_guided_workspace_bytes" : "mh_t5_slots_workspace_bytes");
  MH_TRY(check_arch2_weights(c, w, who));
  hipStream_t s = (hipStream_t)stream;
  int dev = 0;
  MH_TRY(stream_device(s, &dev));
  DeviceGuard device_guard(dev);
  std::unique_ptr<SlotSession> ss(new SlotSession());
  ss->c = c; ss->w = w; ss->S = S; ss->R = R; ss->guided = guided; ss->dev = dev; ss->max_length = sp->max_length; ss->poll_every = poll_every <= 0 ? 16 : poll_every;
  ss->cross_kv = (char*)cross_kv_slots; ss->tokens = tokens;
  ss->cross8 = (uint8_t*)sp->cross_kv_fp8; ss->self8 = (uint8_t*)self_kv_fp8;   // (both NULL behind mh_t5_slots_open)
  slots_layout(c, S, workspace, ss.get(), guided);
  ss->n_chains = guided ? 1 : pick_chains(S);
  ss->rows_per = ceil_div(R, ss->n_chains);
  // every slot idle: position -1, flag set (the recount of n_running counts clear flags); the chains' control blocks zero
  if (hipMemsetAsync(ss->pos, 0xff, (size_t)R * 4, s) != hipSuccess || hipMemsetAsync(ss->plen, 0, (size_t)R * 4, s) != hipSuccess ||
      hipMemsetAsync(ss->ly.bf.finished, 1, (size_t)R, s) != hipSuccess ||
      hipMemsetAsync(ss->mask, 1, (size_t)R * sp->max_length, s) != hipSuccess ||
      hipMemsetAsync(ss->ly.bf.st, 0, (size_t)align256(sizeof(DecState)) * kMaxChains, s) != hipSuccess)
    return check_launch("slot state memset");
  if (hipStreamCreateWithFlags(&ss->admit_stream, hipStreamNonBlocking) != hipSuccess) return check_launch("slot stream create");
  for (int b = 0; b < S; ++b) {
    if (hipEventCreateWithFlags(&ss->freed[b], hipEventDisableTiming) != hipSuccess) return check_launch("slot event create");
    if (hipEventRecord(ss->freed[b], s) != hipSuccess) return check_launch("slot event record");
  }
  const RowSetP rowset{rows, eos_tables, n_eos_sets};
  GenerateArgs a{c, w, cross_kv_slots, R, nullptr, ss->mask, sp->max_length, nullptr, sp, tokens, nullptr, logits_dump, nullptr, workspace,
                 workspace_bytes, poll_every, stream, self_kv_fp8, &rowset, who};
  // prompt_mask: the slot mask rows, stride max_length (call.P); the chains' rows of both e4m3 copies (both pointers are in the key
  // of the step graph: a kv8 session and a plain one never share a graph)
  ss->n_chains = chain_calls(a, ss->ly, ss->n_chains, ss->rows_per, ss->self8, ss->calls);
  for (int ci = 0; ci < ss->n_chains; ++ci) {
    StepCall& call = ss->calls[ci];
    call.slot_pos = ss->pos; call.slot_plen = ss->plen;
    Chain& ch = ss->chains[ci];
    if (hipStreamCreateWithFlags(&ch.stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&ss->admitted[ci], hipEventDisableTiming) != hipSuccess)
      return check_launch("slot stream create");
    ch.st = call.bf.st;
    if (hipStreamWaitEvent(ch.stream, ss->freed[0], 0) != hipSuccess) return check_launch("slot stream wait");   // behind the memsets
    MH_TRY(chain_step_graph(call, who, &ch));
  }
  if (hipStreamSynchronize(s) != hipSuccess) return check_launch("slot open");
  *handle = ss.release();
  return MH_OK;
}
}  // namespace mh

extern "C" int mh_t5_slots_open(const MhT5Config* c, const MhT5Weights* w, int S, const MhSampling* sp, const MhRowSampling* rows,
                                const uint8_t* eos_tables, int n_eos_sets, void* cross_kv_slots, int32_t* tokens, float* logits_dump,
                                const int32_t* forced, void* self_kv_fp8, void* workspace, int64_t workspace_bytes, int poll_every,
                                void* stream, void** handle) {
  return mh::slots_open_impl(c, w, S, sp, rows, eos_tables, n_eos_sets, cross_kv_slots, tokens, logits_dump, forced, self_kv_fp8, workspace,
                             workspace_bytes, poll_every, stream, handle, false, "mh_t5_slots_open");
}

extern "C" int mh_t5_slots_open_kv8(const MhT5Config* c, const MhT5Weights* w, int S, const MhSampling* sp, const MhRowSampling* rows,
                                    const uint8_t* eos_tables, int n_eos_sets, void* cross_kv_slots, int32_t* tokens, float* logits_dump,
                                    const int32_t* forced, void* self_kv_fp8, void* workspace, int64_t workspace_bytes, int poll_every,
                                    void* stream, void** handle) {
  // with neither copy this is mh_t5_slots_open (which then refuses a NULL cross_kv_slots as ever)
  const bool kv8 = (sp && sp->cross_kv_fp8) || self_kv_fp8;
  return mh::slots_open_impl(c, w, S, sp, rows, eos_tables, n_eos_sets, cross_kv_slots, tokens, logits_dump, forced, self_kv_fp8, workspace,
                             workspace_bytes, poll_every, stream, handle, kv8, "mh_t5_slots_open_kv8");
}

extern "C" int mh_t5_slots_open_guided(const MhT5Config* c, const MhT5Weights* w, int S, const MhSampling* sp, const MhRowSampling* rows,
                                       const uint8_t* eos_tables, int n_eos_sets, void* cross_kv_slots, int32_t* tokens, float* logits_dump,
                                       const int32_t* forced, void* self_kv_fp8, void* workspace, int64_t workspace_bytes, int poll_every,
                                       void* stream, void** handle) {
  const bool kv8 = (sp && sp->cross_kv_fp8) || self_kv_fp8;
  return mh::slots_open_impl(c, w, S, sp, rows, eos_tables, n_eos_sets, cross_kv_slots, tokens, logits_dump, forced, self_kv_fp8, workspace,
                             workspace_bytes, poll_every, stream, handle, kv8, "mh_t5_slots_open_guided", true);
}

// mh_t5_slots_admit (one row) and mh_t5_slots_admit_pair (n_rows = 2: `prompt` is [2][P], the negative row first; the rows of the pair
// are decode rows slot and S + slot, one cross K/V row and one mask for both)
static int slots_admit_impl(mh::SlotSession* ss, int slot, const void* cross_kv_row, const int32_t* prompt, const uint8_t* prompt_mask, int P,
                            void* stream, const char* who) {
  using namespace mh;
  OptionScope option_scope(ss->c->options);
  MH_REQUIRE(cross_kv_row && prompt, "%s: null argument", who);
  MH_REQUIRE(slot >= 0 && slot < ss->S, "%s: slot %d not in [0, %d)", who, slot, ss->S);
  MH_REQUIRE(!ss->live[slot], "%s: slot %d is live (release it first)", who, slot);
  MH_REQUIRE(P >= 1 && P < ss->max_length, "%s: prompt length %d must be in [1, max_length)", who, P);
  DeviceGuard device_guard(ss->dev);
  const MhT5Config* c = ss->c;
  const int ci = ss->chain_of(slot), es = es_of(c->dtype), H = c->n_heads, inner = H * 64;
  hipStream_t as = ss->admit_stream;
  if (hipStreamWaitEvent(as, ss->freed[slot], 0) != hipSuccess) return check_launch("admit wait");
  if (stream) {   // the caller's stream wrote cross_kv_row / prompt / prompt_mask: the admission reads them behind that work
    if (!ss->caller_ev && hipEventCreateWithFlags(&ss->caller_ev, hipEventDisableTiming) != hipSuccess) return check_launch("admit event create");
    if (hipEventRecord(ss->caller_ev, (hipStream_t)stream) != hipSuccess || hipStreamWaitEvent(as, ss->caller_ev, 0) != hipSuccess)
      return check_launch("admit caller wait");
  }
  // the window's compact cross K/V [n_dec][2][1][H][L][64] -> row `slot` of [n_dec][2][S][H][L][64]
  const size_t row_bytes = (size_t)H * c->src_len * 64 * es;
  if (ss->cross_kv && hipMemcpy2DAsync(ss->cross_kv + (size_t)slot * row_bytes, (size_t)ss->S * row_bytes, cross_kv_row, row_bytes, row_bytes,
                                       (size_t)c->n_dec_layers * 2, hipMemcpyDeviceToDevice, as) != hipSuccess)
    return check_launch("admit cross K/V copy");
  // ... and, quantised, -> row `slot` of the S-row e4m3 copy (bytes and scales; no other row is touched)
  if (ss->cross8) MH_TRY(launch_cross_kv_quant_row(c, ss->S, cross_kv_row, ss->cross8, slot, as));
  const int n_rows = ss->guided ? 2 : 1;
  const int row[2] = {slot, ss->S + slot};   // (a plain session: row[0] alone)
  for (int j = 0; j < n_rows; ++j) {
    int32_t* trow = ss->tokens + (long)row[j] * ss->max_length;
    uint8_t* mrow = ss->mask + (long)row[j] * ss->max_length;
    if (hipMemcpyAsync(trow, prompt + (long)j * P, (size_t)P * 4, hipMemcpyDeviceToDevice, as) != hipSuccess) return check_launch("admit prompt copy");
    if (hipMemsetAsync(mrow, 1, (size_t)ss->max_length, as) != hipSuccess) return check_launch("admit mask set");
    if (prompt_mask && hipMemcpyAsync(mrow, prompt_mask, (size_t)P, hipMemcpyDeviceToDevice, as) != hipSuccess) return check_launch("admit mask copy");
  }
  int start_pos = 0;
  if (P > 1 && option(OPT_DECODE_PREFILL) != 0) {   // positions 0 .. P-2 into the slot's cache rows: the B = 1 prefill of a uniform call
    PrefillBuf pb;
    prefill_layout(c, 1, P - 1, ss->prefill_base, ss->prefill_bytes, &pb);
    start_pos = P - 1;
    // (a pair: one row after the other through the same buffers, each as a row block of the B = 2 prefill of the guided call -- the
    // GEMM kernels that call would run, so the cache rows hold its bits)
    for (int j = 0; j < n_rows; ++j) {
      const long cache_row = (long)row[j] * inner * c->tgt_len * es;
      MH_TRY(prefill_prompt(c, ss->w, cross_kv_row, 1, 1, prompt + (long)j * P, prompt_mask, P, P - 1, (char*)ss->ly.bf.self_k + cache_row,
                            (char*)ss->ly.bf.self_v + cache_row, pb, as, ss->R, n_rows));
      // the prefilled positions 0 .. P-2 of the slot's cache rows -> the same places of the R-row shadow, every layer, k and v (the pass a
      // uniform call makes after its prefill); nothing else of the shadow is written
      if (ss->self8) MH_TRY(launch_self_kv_quant_slot(c, ss->R, ss->ly.bf, ss->self8, row[j], start_pos, as));
    }
  }
  const SampleP& smp = ss->calls[ci].smp;
  for (int j = 0; j < n_rows; ++j)   // (a pair: the negative row, then the prompt row -- the positions stay the last words written)
    MH_TRY(launch_dec_slot_init(c->dtype, smp, row[j], P, start_pos, ss->pos, ss->plen, as));
  if (hipEventRecord(ss->admitted[ci], as) != hipSuccess) return check_launch("admit record");
  ss->pending[ci] = true;
  ss->live[slot] = true;
  return MH_OK;
}

extern "C" int mh_t5_slots_admit(void* handle, int slot, const void* cross_kv_row, const int32_t* prompt, const uint8_t* prompt_mask, int P,
                                 void* stream) {
  mh::SlotSession* ss = (mh::SlotSession*)handle;
  const char* who = "mh_t5_slots_admit";
  MH_REQUIRE(ss, "%s: null handle", who);
  MH_REQUIRE(!ss->guided, "%s: the session is guided (mh_t5_slots_open_guided): its slots are pairs, admitted by mh_t5_slots_admit_pair", who);
  return slots_admit_impl(ss, slot, cross_kv_row, prompt, prompt_mask, P, stream, who);
}

extern "C" int mh_t5_slots_admit_pair(void* handle, int slot, const void* cross_kv_row, const int32_t* prompt_pair, const uint8_t* prompt_mask,
                                      int P, void* stream) {
  mh::SlotSession* ss = (mh::SlotSession*)handle;
  const char* who = "mh_t5_slots_admit_pair";
  MH_REQUIRE(ss, "%s: null handle", who);
  MH_REQUIRE(ss->guided, "%s: the session is not guided (mh_t5_slots_open_guided opens one): its slots are rows, admitted by mh_t5_slots_admit", who);
  return slots_admit_impl(ss, slot, cross_kv_row, prompt_pair, prompt_mask, P, stream, who);
}

extern "C" int mh_t5_slots_run(void* handle, int n_steps, uint8_t* finished_out, int32_t* length_out, int32_t* steps_out) {
  using namespace mh;
  SlotSession* ss = (SlotSession*)handle;
  const char* who = "mh_t5_slots_run";
  MH_REQUIRE(ss, "%s: null handle", who);
  OptionScope option_scope(ss->c->options);
  MH_REQUIRE(n_steps >= 0 && finished_out && length_out, "%s: bad argument", who);
  DeviceGuard device_guard(ss->dev);
  int steps[kMaxChains] = {}, which[kMaxChains], n_run = 0;   // which: the chains with a live slot run
  bool runs[kMaxChains] = {};
  for (int b = 0; b < ss->S; ++b) if (ss->live[b]) runs[ss->chain_of(b)] = true;
  for (int ci = 0; ci < ss->n_chains; ++ci) {
    if (!runs[ci]) continue;
    which[n_run++] = ci;
    // The fused tail's hand-off counters only ever grow inside a call, and a launch takes its base as a multiple of its grid: a
    // session has no dec_init_kernel between its steps, so they start every run at zero (the chain is idle here: the last run
    // ended with its poll) and cannot wrap however long the session lives.  tail_err stays: a timed-out session stays reported.
    if (n_steps > 0 && hipMemsetAsync(ss->chains[ci].st->tail_cnt, 0, sizeof(ss->chains[ci].st->tail_cnt), ss->chains[ci].stream) != hipSuccess)
      return check_launch("tail counter reset");
    if (ss->pending[ci]) {   // the step that first sees the admitted slots live waits for their admissions
      if (hipStreamWaitEvent(ss->chains[ci].stream, ss->admitted[ci], 0) != hipSuccess) return check_launch("admission wait");
      ss->pending[ci] = false;
    }
  }
  int rc = n_steps > 0 ? launch_chains(ss->chains, which, n_run, n_steps, ss->poll_every, true, who, steps) : MH_OK, total = 0;
  for (int ci = 0; ci < ss->n_chains; ++ci) total += steps[ci];
  // one poll per chain: its rows' flags, finish columns and positions, and the bounded hand-offs' last word
  for (int ci = 0; ci < ss->n_chains; ++ci) {
    const int b0 = ci * ss->rows_per, n = ss->calls[ci].Bc;
    hipStream_t cs = ss->chains[ci].stream;
    int word[2] = {0, 0};
    if (hipMemcpyAsync(ss->host_fin + b0, ss->ly.bf.finished + b0, (size_t)n, hipMemcpyDeviceToHost, cs) != hipSuccess ||
        hipMemcpyAsync(ss->host_col + b0, ss->ly.bf.finish_col + b0, (size_t)n * 4, hipMemcpyDeviceToHost, cs) != hipSuccess ||
        hipMemcpyAsync(ss->host_pos + b0, ss->pos + b0, (size_t)n * 4, hipMemcpyDeviceToHost, cs) != hipSuccess ||
        hipMemcpyAsync(word, &ss->chains[ci].st->n_running, 8, hipMemcpyDeviceToHost, cs) != hipSuccess ||
        hipStreamSynchronize(cs) != hipSuccess)
      return check_launch("slot poll");
    if (rc == MH_OK && word[1] != 0) rc = mh_t5_decode_tail_status(word[1]);
  }
  for (int b = 0; b < ss->S; ++b) {   // (a pair: read from its prompt row)
    const int r = ss->row_of(b);
    const bool fin = ss->live[b] && ss->host_fin[r] != 0;
    finished_out[b] = fin ? 1 : 0;
    length_out[b] = !ss->live[b] ? 0 : (fin ? ss->host_col[r] + 1 : ss->host_pos[r] + 1);
  }
  if (steps_out) *steps_out = total;
  return rc;
}

extern "C" int mh_t5_slots_release(void* handle, int slot) {
  using namespace mh;
  SlotSession* ss = (SlotSession*)handle;
  const char* who = "mh_t5_slots_release";
  MH_REQUIRE(ss, "%s: null handle", who);
  MH_REQUIRE(slot >= 0 && slot < ss->S, "%s: slot %d not in [0, %d)", who, slot, ss->S);
  MH_REQUIRE(ss->live[slot], "%s: slot %d is idle", who, slot);
  DeviceGuard device_guard(ss->dev);
  const int ci = ss->chain_of(slot);
  hipStream_t cs = ss->chains[ci].stream;
  if (ss->pending[ci]) {   // released before a step saw it: still behind its own admission
    if (hipStreamWaitEvent(cs, ss->admitted[ci], 0) != hipSuccess) return check_launch("admission wait");
    ss->pending[ci] = false;
  }
  // on the chain's stream, behind the slot's last step: idle again (negative position, flag set), then the event an admission waits for
  if (hipMemsetAsync(ss->pos + slot, 0xff, 4, cs) != hipSuccess || hipMemsetAsync(ss->ly.bf.finished + slot, 1, 1, cs) != hipSuccess)
    return check_launch("slot release");
  if (ss->guided && (hipMemsetAsync(ss->pos + ss->S + slot, 0xff, 4, cs) != hipSuccess ||   // both rows of the pair
                     hipMemsetAsync(ss->ly.bf.finished + ss->S + slot, 1, 1, cs) != hipSuccess))
    return check_launch("slot release");
  if (hipEventRecord(ss->freed[slot], cs) != hipSuccess) return check_launch("slot release");
  ss->live[slot] = false;
  return MH_OK;
}

extern "C" int mh_t5_slots_close(void* handle) {
  using namespace mh;
  SlotSession* ss = (SlotSession*)handle;
  if (!ss) return MH_OK;
  DeviceGuard device_guard(ss->dev);
  delete ss;   // joins the chains, then releases the graph references (the cross-call cache keeps the graphs it owns)
  return check_launch("slot close");
}

extern "C" int mh_t5_decode_chains(int B) { return B > 0 ? mh::pick_chains(B) : 0; }
extern "C" int mh_t5_decode_chains_cfg(const MhT5Config* c, int B) {   // ... under the engine's option set
  mh::OptionScope option_scope(c ? c->options : nullptr);
  return B > 0 ? mh::pick_chains(B) : 0;
}
