// runtime_resident.hip — the device-resident LLaMA loops (extension; see include/zgml_hip.h): set-up; the greedy loops
// (single-sequence decode, batched decode, the prefill chunk); their sampled forms and the sampled / greedy speculative verify
// loop — also with a second resident program drafting inside the step (zgml_hip_resident_decode_speculative_model) —, and the greedy / sampled verify loop of every sequence of a batched plan — also with a batched
// draft program (zgml_hip_resident_decode_batch_speculative_model) —; the blocking calls over one buffer range
// (zgml_hip_sample, zgml_hip_logprobs, zgml_hip_top_logprobs) with their result
// getters; the token constraint's create / attach / state. Everything a step needs (embedding row, mask column, RoPE rows, the
// dynamic words) is produced on the device from a few state words, so a call is a train of launches (or graph replays) with one
// copy-out at the end. The loops share one skeleton: resident_begin, the per-step lambda (captured once: capture_once, then
// replay), resident_end; what follows the plan in a sampled step is stated once, by SampledTail.
// The state they run over owns itself: every device block is a DevBlock (dev_block.h: pointer + the count it was allocated
// for, freed by its destructor, allocated in all-or-nothing groups by ensure_blocks / grow_tables below) and every captured
// graph a GraphSlot (runtime_internal.h), so a new field is declared once and remembered nowhere else.
// No kernels here: the prep / pick kernels are in greedy_tail.hip, the plan's and the sampled tail's in their own files.
#include "runtime_internal.h"
#include <atomic>
#include "sample.h"
#include "sample_params.h"
#include "spec.h"

// the forms of the sampled loops' step: the select launch (SampledSel, kernels.h), and what follows the pick. The constrained
// select kernel serves rows with and without penalties, so a constrained call has one graph per kind
enum SampledKind { kKindPick, kKindLogprobs, kKindTop, kSampledKinds };
constexpr uint32_t kSampledForms = kSampledSels * kSampledKinds;
constexpr uint32_t sampled_form(uint32_t sel, uint32_t kind) { return kind * kSampledSels + sel; }
// the names the graphs are captured under: prefix + one of these
static const char* const kSampledFormNames[kSampledForms] = {"sampled", "penalized", "constrained", "constrained_rows",
                                                             "sampled_logprobs", "penalized_logprobs", "constrained_logprobs", "constrained_rows_logprobs",
                                                             "sampled_top", "penalized_top", "constrained_top", "constrained_rows_top"};

// an uploaded token automaton (zgml_hip_constraint_create)
struct zgml_hip_constraint {
    uint32_t n_states = 0, n_classes = 0, vocab = 0;
    uint32_t attached = 0; // sequences it is attached to: it is not freed before that is 0
    DevBlock<uint16_t> class_of, next;
    DevBlock<uint32_t> forced; // [n_states]: the state's only allowed token or kConstraintNoForced (sample.h)
};

// The resident set-up of a program. Every device block below is owned by its field (DevBlock: the count it was allocated for is
// its capacity, deleting the set-up frees it) and every graph by its slot; what is not allocated by the set-up itself is
// allocated by the first call that needs it, as one group (ensure_blocks), and a block sized by the rows of that first call
// refuses a later call with more (block_holds). The tables next to the produced tokens grow (grow_tables), which drops the graphs.
struct zgml_resident {
    DevBlock<float> embed, cos, sin;
    uint32_t vocab = 0, d = 0, max_seq = 0, dh = 0, n_rope = 0;
    float *tok_in = nullptr, *mask = nullptr, *logits = nullptr; // (the program's buffers: not owned)
    DevBlock<float*> rope_bufs;   // device array of n_rope pointers
    DevBlock<uint32_t> dyn_kind;  // per op: 0 static, 1 store (base + pos * stride), 2 attention (pos + T) — dyn_field's roles, for the prep kernels
    DevBlock<uint32_t> dyn_base;
    DevBlock<uint32_t> dyn_stride;
    DevBlock<uint32_t> state;     // [0] token, [1] pos, [2] produced count
    uint32_t token_len = 1;        // T of the plan (token_input holds T rows): 1 = decode, > 1 = prefill chunk
    DevBlock<uint32_t> tok_dev;   // prefill: the chunk's T token ids (the only per-chunk host -> device traffic)
    DevBlock<int64_t> tokens;     // produced tokens (device), grown by grow_tables: the graphs bake pointer and capacity (its count)
    uint32_t tokens_cap() const { return (uint32_t)tokens.count(); }
    uint32_t prep_total = 0;       // the prep launches' flat index space (prep_total(): fixed by the set-up, which checks that it fits)
    uint32_t tail_launches = 0;    // launches behind the plan in a step of the single-sequence greedy loop, as its step last ran (or was captured)
    GraphSlot graph;               // the greedy loop's step: single-sequence, batched or verify, whichever the plan is
    GraphSlot graph_multi;         // `multi_n` consecutive tokens as one graph (ZGML_HIP_RESIDENT_TOKENS_PER_GRAPH)
    uint32_t multi_n = 0;
    // batched program (zgml_hip_program_set_sequences): per-sequence device state (kernels.h: ResidentBatchPrepArgs), the sequence of
    // every dynamic op, the pick's scratch (n_seqs rows of partial maxima) and the produced tokens [n_seqs][steps] (grown as `tokens`)
    uint32_t n_seqs = 0;
    DevBlock<uint32_t> bstate;
    DevBlock<uint32_t> dyn_seq;
    DevBlock<float> bval;
    DevBlock<int64_t> bidx;
    DevBlock<int64_t> btokens;
    // speculative loop over a token_len > 1 plan (zgml_hip_resident_decode_speculative), allocated by its first call: the state
    // words (kernels.h: SpecWord), the token at every position, the provided drafts (max_seq words each: a position past max_seq
    // is never drafted); the T candidates are tok_dev, the rows' partial maxima bval / bidx, the produced tokens `tokens`
    DevBlock<uint32_t> spec;
    DevBlock<uint32_t> hist;
    DevBlock<uint32_t> drafts;
    DevBlock<uint32_t> picks; // the sampled form's token of every logits row, [T] (zgml_hip_resident_decode_speculative_sampled)
    // speculative loop over a batched plan with tokens_per_seq = Ts >= 2 columns per sequence (token_len = n_seqs * Ts;
    // zgml_hip_resident_decode_batch_speculative), allocated by its first call: per sequence the state words, then one word, the row
    // length of the call's token table (kernels.h: SpecBatchArgs); the history rows [n_seqs][max_seq + 1]; the provided drafts
    // [n_seqs][max_seq]. The candidates are tok_dev, the rows' partial maxima bval / bidx, the produced tokens btokens. The step's
    // graph is its own: no other loop runs on such a plan, and no other call's graph is dropped for it
    uint32_t tokens_per_seq = 1;
    DevBlock<uint32_t> bspec;
    DevBlock<uint32_t> bhist;
    DevBlock<uint32_t> bdrafts;
    GraphSlot bspec_graph;
    // sampled tail (zgml_hip_resident_decode_sampled / _batch_sampled / _speculative_sampled), allocated by the first such call: one
    // parameter row and one set of partial candidate lists per sequence (per logits row of a token_len > 1 plan, whose verify
    // step reads parameter row 0 alone). sparams' count is the rows both were allocated for
    DevBlock<SampleParamsDev> sparams;
    DevBlock<uint64_t> skeys;
    // The sampled loops' graphs, one per form — what the select launch is (SampledSel) times what follows the pick (SampledKind):
    // the forms alternate on one program and invalidate nothing, and the greedy loop's graph stays valid beside them.
    // SampledTail::form() indexes them
    GraphSlot sgraph[kSampledForms];
    // penalised sampled tail (sample.h: the penalties), allocated by the first penalised or constrained call of the single or the
    // batched loop: the window of every sequence, [n_seqs][256] token words indexed by position & 255, then lo per sequence (the
    // verify step reads hist / cand instead)
    DevBlock<uint32_t> swin;
    // log-probabilities of the sampled tail (the `logprobs` field of zgml_sampling; logprob.hip), allocated by the first such call:
    // the block pairs of every logits row, the values next to the produced tokens (the layout and count of tokens / btokens), the
    // T row values of a verify step (its count: the rows the three were allocated for), the "written up to" word of every sequence
    DevBlock<float> lpart, lp, lp_rows;
    DevBlock<uint32_t> lp_written;
    // the alternatives of the sampled tail (the `top_logprobs` word of zgml_sampling; top_logprob.hip), allocated by the first such
    // call: the lists of a select over the RAW rows (what a penalised or constrained step needs beside skeys, the same size), the
    // pairs next to the produced tokens ([count of the tokens][64], the layout of lp), the T rows' pairs of a verify step
    DevBlock<uint64_t> skeys_raw;
    DevBlock<uint32_t> top_tok, top_rows_tok;
    DevBlock<float> top_val, top_rows_val;
    // constrained sampled tail (sample.h: THE CONSTRAINT; zgml_hip_program_set_constraint), allocated by the first attachment: what
    // is attached to every sequence (one entry for a plain plan), the device table the kernels read (kernels.h:
    // SampleConstraintRow, uploaded at every attach / detach) and the sequences' state words, which the merge launch advances
    std::vector<zgml_hip_constraint*> con;
    uint32_t n_con = 0; // attached sequences
    DevBlock<SampleConstraintRow> con_rows;
    DevBlock<uint32_t> con_state;
    // constrained verify step (zgml_hip_resident_decode_speculative_constrained), allocated by its first call: the state of every
    // logits row, [T] (spec.h: UNDER A CONSTRAINT) — the draft launch writes them, the constrained-rows select launch reads them —,
    // [n_seqs * tokens_per_seq] on a batched plan (zgml_hip_resident_decode_batch_speculative_constrained)
    DevBlock<uint32_t> row_state;
    // speculative decode with a draft model (zgml_hip_resident_decode_speculative_model; on a batched plan
    // zgml_hip_resident_decode_batch_speculative_model, the only call that can use the slots there), on the TARGET's set-up: the step's graphs
    // hold the launches of two programs, so they belong to the pair — pair_draft and the draft set-up's graph_epoch as it stood at
    // the capture; another draft, or one whose epoch moved, re-captures —, one per form ([0] greedy, [1 + SampledTail::form()]
    // the sampled ones) and apart from every other slot: other calls on either program alternate with the pair's and drop nothing
    zgml_hip_program* pair_draft = nullptr;
    uint64_t pair_epoch = 0;
    GraphSlot pair_graph[1 + kSampledForms];
    // what a graph that bakes THIS set-up's launches is valid for: a process-wide count, taken at the set-up and again whenever
    // its graphs are dropped (free_resident_graph: a plan rebuild, a grown table), so no two states of any program share a value —
    // a program created at a freed one's address included
    uint64_t graph_epoch = 0;
};
using Resident = zgml_resident;

namespace zgml_rt {

static std::atomic<uint64_t> g_graph_epoch{0}; // (Resident::graph_epoch)

// the pair's graphs on the target's set-up (Resident::pair_graph)
static void free_pair_graphs(Resident* r) {
    for (GraphSlot& g : r->pair_graph) g.reset();
    r->pair_draft = nullptr, r->pair_epoch = 0;
}

void free_resident_graph(zgml_hip_program* p) {
    Resident* r = p->resident;
    if (!r) return;
    r->graph_epoch = ++g_graph_epoch; // (a pair graph on ANOTHER program that bakes this one as its draft is stale from here on)
    free_pair_graphs(r);
    r->graph.reset(), r->graph_multi.reset(), r->multi_n = 0, r->bspec_graph.reset();
    for (GraphSlot& g : r->sgraph) g.reset();
}

void free_resident(zgml_hip_program* p) {
    Resident* r = p->resident;
    if (!r) return;
    free_resident_graph(p);
    for (zgml_hip_constraint* c : r->con)
        if (c) c->attached -= 1; // (a program that goes detaches its sequences)
    delete r; // (every block with it)
    p->resident = nullptr;
}

bool has_constraint(const zgml_hip_program* p) { return p && p->resident && p->resident->n_con != 0; }

} // namespace zgml_rt

namespace {

// what the entry points that would pick tokens while ignoring an attached constraint say (include/zgml_hip.h); true: refused
bool refuse_constrained(zgml_hip_ctx* ctx, const zgml_hip_program* p, const char* who) {
    if (!has_constraint(p)) return false;
    ctx->fail(std::string(who) + ": a constraint is attached to the program (only zgml_hip_resident_decode_sampled, _batch_sampled, zgml_hip_resident_decode_speculative_constrained and zgml_hip_sample honour one: detach it first)");
    return true;
}

// the batched loops that advance one token per sequence and step, on a plan with several columns per sequence; true: refused
bool refuse_verify_plan(zgml_hip_ctx* ctx, const Resident* r, const char* who) {
    if (r->tokens_per_seq <= 1) return false;
    ctx->fail(std::string(who) + ": the batched plan holds " + std::to_string(r->tokens_per_seq) +
              " columns per sequence (tokens_per_seq > 1: zgml_hip_resident_decode_batch_speculative runs it)");
    return true;
}

// the constraint arguments of a sampled launch over the program's sequences (none attached: no rows, the other launches)
SampleConstraint constraint_args(const Resident* r) {
    SampleConstraint c;
    if (r->n_con) c.rows = r->con_rows, c.state = r->con_state;
    return c;
}

// would every moving op stay inside the bounds the batched plan assumed with its sequence at position pos_of(op index), T token
// rows per step? (The device patches the words itself, resident_prep_kernel: nothing else would notice a position outside them.)
template <class PosOf>
bool positions_in_bounds(const zgml_hip_program* p, uint32_t T, PosOf pos_of) {
    for (const uint32_t i : p->dyn_ops) {
        zgml_device_op o = p->ops[i];
        const DynField f = dyn_field(o);
        *f.word = f.at(pos_of(i), T);
        if (!dynamic_field_in_bounds(p->sched, i, o)) return false;
    }
    return true;
}

// what every loop does before it enqueues anything: the plan is current; when it is a batched plan and `in_bounds()` says this
// call's positions leave its bounds, program order for good, like refresh_program; then the static dyn words (row stores with
// patch_stride 0) go up from the host mirror — the prep kernels only rewrite the position-dependent ones
template <class InBounds>
void resident_begin(zgml_hip_program* p, InBounds in_bounds) {
    ensure_plan(p);
    if (p->plan_batched && !in_bounds()) {
        p->batching_safe = false;
        free_graph(p);
        build_plan(p);
    }
    set_dyn_from_ops(p);
    p->dyn_dirty = true;
    flush_dyn(p);
}

// ... and after its last synchronisation: the device rewrote the dyn block behind the host mirror's back, so the mirror is
// invalidated to force a re-upload next time; `steps` executions of `launches_per_step` launches go into the profile
void resident_end(zgml_hip_program* p, uint64_t steps, uint64_t launches_per_step) {
    memset(p->dyn_host, 0xFF, p->ops.size() * sizeof(uint32_t));
    set_dyn_from_ops(p);
    p->dyn_dirty = true;
    p->profile.call_count += steps;
    p->profile.backend_op_count += steps * p->ops.size();
    p->profile.backend_dispatch_count += steps * launches_per_step;
}

// which entry point's rules the `recent` tokens of a zgml_sampling are held to (include/zgml_hip.h)
enum class RecentOf { Sample, Loop, Spec };

// a caller's zgml_sampling as the kernels read it; false (with the error on the context) for what the header refuses.
// vocab == 0: the stop tokens are not looked at (zgml_hip_sample). start_pos: of the sequence, for the loops' n_recent rule.
// row_len: the logits of a row, for the `logprobs` field's limit
bool sampling_params(zgml_hip_ctx* ctx, const std::string& who, const zgml_sampling* sp, uint32_t vocab, uint64_t row_len, SampleParamsDev* out,
                     RecentOf form = RecentOf::Sample, uint32_t start_pos = 0) {
    if (!sp) {
        ctx->fail(who + ": no sampling parameters");
        return false;
    }
    if (!(sp->temperature > 0.0f) || !(sp->top_p > 0.0f && sp->top_p <= 1.0f)) {
        ctx->fail(who + ": temperature must be > 0 and top_p in (0, 1]");
        return false;
    }
    if (sp->top_k > kSampleMaxK || sp->n_stop > kSampleMaxStop) {
        ctx->fail(who + ": top_k must be at most " + std::to_string(kSampleMaxK) + " and n_stop at most " + std::to_string(kSampleMaxStop));
        return false;
    }
    for (uint32_t i = 0; vocab && i < sp->n_stop; i++)
        if (sp->stop[i] >= vocab) {
            ctx->fail(who + ": stop token out of range");
            return false;
        }
    // the penalties: pure host logic in a header of its own, so that a CPU test can hold it to the list in include/zgml_hip.h
    float repeat = 1.0f;
    uint32_t active = 0;
    if (const char* why = sample_penalty_check(sp, form == RecentOf::Loop ? 1 : form == RecentOf::Spec ? 2 : 0, vocab, start_pos, &repeat, &active)) {
        ctx->fail(who + ": " + why);
        return false;
    }
    if (const char* why = sample_logprobs_check(sp, row_len)) {
        ctx->fail(who + ": " + why);
        return false;
    }
    *out = SampleParamsDev{1.0f / sp->temperature, sp->top_p, sp->top_k, vocab ? sp->n_stop : 0, {sp->stop[0], sp->stop[1], sp->stop[2], sp->stop[3]},
                           sp->stream, (uint32_t)sp->seed, (uint32_t)(sp->seed >> 32),
                           repeat, 1.0f / repeat, sp->presence_penalty, sp->frequency_penalty, sp->penalty_window, active, sample_top_logprobs(sp)};
    return true;
}

// what a call uploads into the window block of the penalised loops ([rows][256] ring words, then lo per row) for sequence b of `rows`: the last W - 1 of its recent tokens at their positions' slots
// (the token at start_pos and every later one is filed by the select launch itself), and lo
void fill_window_block(std::vector<uint32_t>& block, uint32_t rows, uint32_t b, const zgml_sampling& sp, uint32_t start_pos) {
    const uint32_t W = sp.penalty_window, take = W ? std::min(sp.n_recent, W - 1) : 0;
    for (uint32_t i = 0; i < take; i++) {
        const uint32_t q = start_pos - take + i;
        block[(size_t)b * kSamplePenaltyMaxWindow + (q & (kSamplePenaltyMaxWindow - 1))] = sp.recent[sp.n_recent - take + i];
    }
    block[(size_t)rows * kSamplePenaltyMaxWindow + b] = start_pos - sp.n_recent;
}

// The one way the loops and the blocking calls get their device blocks, named as (block, count) pairs. Nothing happens when
// every block holds its count. Else the stream is waited for — a block about to be freed may still be read, by a graph too —
// and the group is allocated whole or not at all (dev_block.h: dev_ensure): a failed call leaves every block of it empty, so no
// later call finds the first and takes the rest for granted. `p`: the program whose resident graphs bake the blocks' pointers
// (nullptr: the context's scratch, which no graph bakes): they are dropped when the call failed and, with `baked`, when a pointer moved
template <class... A>
bool ensure_group(zgml_hip_ctx* ctx, zgml_hip_program* p, bool baked, A&&... a) {
    if (dev_holds(a...)) return true;
    hipStreamSynchronize(ctx->stream);
    bool moved = false;
    const bool ok = dev_ensure(&moved, a...);
    if (!ok) ctx->fail(std::string("a device block could not be allocated: ") + hipGetErrorString(hipGetLastError()));
    if (p && moved && (baked || !ok)) free_resident_graph(p);
    return ok;
}
// blocks allocated by the first call that needs them: no graph of an earlier call can hold their pointers
template <class... A>
bool ensure_blocks(zgml_hip_ctx* ctx, zgml_hip_program* p, A&&... a) {
    return ensure_group(ctx, p, false, a...);
}
// the tables that lie next to the produced tokens (tokens / btokens, the values, the pairs) with room for this call. The graphs
// bake pointer and capacity: growing one drops them
template <class... A>
bool grow_tables(zgml_hip_ctx* ctx, zgml_hip_program* p, A&&... a) {
    return ensure_group(ctx, p, true, a...);
}

// A scratch block that exists was sized by the first call that needed it. Every loop of one program asks for the same rows
// today (the plan fixes them), but a launch over more rows than the block holds would write out of bounds on the device: refused
// here, on the host
bool block_holds(zgml_hip_ctx* ctx, const char* what, size_t have, uint32_t rows) {
    if (have >= rows) return true;
    ctx->fail(std::string(what) + " were allocated for " + std::to_string(have) + " logits rows, this call needs " + std::to_string(rows));
    return false;
}
// ... so every group sized by rows comes through here: `have`, the rows it holds (0: not allocated yet)
template <class... A>
bool ensure_row_blocks(zgml_hip_ctx* ctx, zgml_hip_program* p, const char* what, size_t have, uint32_t rows, A&&... a) {
    return (!have || block_holds(ctx, what, have, rows)) && ensure_blocks(ctx, p, a...);
}

// the window block of the penalised loops: [rows][256] ring words, then lo per row
bool ensure_window_block(zgml_hip_ctx* ctx, zgml_hip_program* p, uint32_t rows) {
    Resident* r = p->resident;
    return ensure_row_blocks(ctx, p, "the penalty windows", r->swin.count() / (kSamplePenaltyMaxWindow + 1), rows, r->swin, (size_t)rows * (kSamplePenaltyMaxWindow + 1));
}

// the sampled loops' device blocks: `rows` parameter rows and partial candidate lists
bool ensure_sample_blocks(zgml_hip_ctx* ctx, zgml_hip_program* p, uint32_t rows) {
    Resident* r = p->resident;
    return ensure_row_blocks(ctx, p, "the sampled tail's blocks", r->sparams.count(), rows, r->sparams, rows, r->skeys, sample_scratch_keys(r->vocab, rows));
}

// the log-probability blocks of the sampled loops: `rows` logits rows, and the values next to the produced tokens of `table`
bool ensure_logprob_blocks(zgml_hip_ctx* ctx, zgml_hip_program* p, uint32_t rows, const DevBlock<int64_t>& table) {
    Resident* r = p->resident;
    return ensure_row_blocks(ctx, p, "the log-probability blocks", r->lp_rows.count(), rows, r->lpart, (size_t)rows * logprob_blocks(r->vocab) * 2, r->lp_rows, rows,
                             r->lp_written, rows) &&
           grow_tables(ctx, p, r->lp, table.count());
}

// the blocks of the alternatives of the sampled loops: `rows` logits rows, and the pairs next to the produced tokens of `table`
bool ensure_top_blocks(zgml_hip_ctx* ctx, zgml_hip_program* p, uint32_t rows, const DevBlock<int64_t>& table) {
    Resident* r = p->resident;
    return ensure_row_blocks(ctx, p, "the alternatives' blocks", r->top_rows_tok.count() / kTopLogprobsMax, rows, r->skeys_raw, sample_scratch_keys(r->vocab, rows),
                             r->top_rows_tok, (size_t)rows * kTopLogprobsMax, r->top_rows_val, (size_t)rows * kTopLogprobsMax) &&
           grow_tables(ctx, p, r->top_tok, table.count() * kTopLogprobsMax, r->top_val, table.count() * kTopLogprobsMax);
}

// the context's blocks of zgml_hip_logprobs (and of zgml_hip_sample with the field) for `rows` rows
bool ensure_ctx_logprob(zgml_hip_ctx* ctx, uint32_t rows) {
    return ensure_blocks(ctx, nullptr, ctx->lp_part, (size_t)rows * kLogprobMaxBlocks * 2, ctx->lp_tok, rows, ctx->lp_out, rows);
}

// the context's blocks of zgml_hip_top_logprobs (and of zgml_hip_sample with the word) for `rows` rows and `keys` list words
bool ensure_ctx_top(zgml_hip_ctx* ctx, uint32_t rows, uint64_t keys) {
    return ensure_blocks(ctx, nullptr, ctx->top_keys, keys, ctx->top_tok, (size_t)rows * kTopLogprobsMax, ctx->top_val, (size_t)rows * kTopLogprobsMax);
}

// Once a call has enqueued a copy that reads its own stack or heap memory (the state words, the parameter rows, a window), a
// failure must not return under it: every loop leaves through here from then on
int fail_after_copies(hipStream_t s) {
    hipStreamSynchronize(s);
    return -1;
}

// What zgml_hip_top_logprobs_result hands out, from a call's downloaded pairs (rows of kTopLogprobsMax, as the device holds
// them): [entries][width], entry e from row src(e), or padding throughout where src(e) < 0 — a token that was not produced, a
// sequence without the word
template <class Src>
void top_keep(zgml_hip_ctx* ctx, uint64_t entries, uint32_t width, const std::vector<uint32_t>& tok, const std::vector<float>& val, Src src) {
    ctx->top_width_last = width;
    ctx->top_tok_last.assign((size_t)entries * width, -1);
    ctx->top_val_last.assign((size_t)entries * width, sample_bits_f32(kLogprobNaNBits));
    for (uint64_t e = 0; e < entries; e++) {
        const int64_t from = src(e);
        if (from < 0) continue;
        for (uint32_t j = 0; j < width; j++) {
            const uint32_t t = tok[(size_t)from * kTopLogprobsMax + j];
            if (t == 0xFFFFFFFFu) continue; // (behind the row's own count)
            ctx->top_tok_last[(size_t)e * width + j] = (int64_t)t;
            ctx->top_val_last[(size_t)e * width + j] = val[(size_t)from * kTopLogprobsMax + j];
        }
    }
}

// entries of tokens that were not produced
void logprob_fill_unproduced(float* out, uint64_t from, uint64_t to) {
    const float nan = sample_bits_f32(kLogprobNaNBits);
    for (uint64_t i = from; i < to; i++) out[i] = nan;
}

// What follows the plan in a sampled step, over `rows` logits rows:
//   ([partial]) [select | penalised select | constrained select] [merge + pick] ([finish], or ([raw select]) [finish + top])
// `sel` and `kind` decide the train, the graph slot and the launch count; the rest is where the launches read and write. The
// single loop, the batched loop, the sampled verify step and zgml_hip_sample each fill one and call launch().
struct SampledTail {
    uint32_t rows = 1;
    SampledSel sel = kSelPlain;
    SampledKind kind = kKindPick;
    uint64_t* keys = nullptr;     // the pick's partial candidate lists
    uint64_t* keys_raw = nullptr; // ... and those of a select over the raw rows (kKindTop with raw_select())
    const SampleParamsDev* params = nullptr;
    float* part = nullptr;        // block pairs of [partial] (kKindLogprobs, kKindTop)
    SampleAdvance adv;
    SampleWindow win;     // (kSelPenalized, kSelConstrained)
    SampleConstraint con; // (kSelConstrained)
    TopLogprobTarget top; // top.chosen is [finish]'s target (kKindLogprobs, kKindTop); the rest [finish + top]'s (kKindTop)

    static SampledSel sel_of(bool constrained, bool penalized) { return constrained ? kSelConstrained : penalized ? kSelPenalized : kSelPlain; }
    static SampledKind kind_of(bool lp, bool top) { return top ? kKindTop : lp ? kKindLogprobs : kKindPick; } // (top: only with lp)
    // penalised or masked lists are not the raw row's: the alternatives then need a select of their own
    bool raw_select() const { return sel != kSelPlain; }
    uint32_t form() const { return sampled_form(sel, kind); }
    // for resident_end: [select] [merge + pick], [partial] and [finish] with log-probabilities, the raw [select] where needed
    uint32_t launches() const { return 2 + (kind != kKindPick ? 2 : 0) + (kind == kKindTop && raw_select() ? 1 : 0); }
    void launch(hipStream_t st, const float* logits, uint64_t vocab) const {
        if (kind != kKindPick) launch_logprob(st, logits, vocab, rows, part); // (the raw row: it depends on the plan alone)
        launch_sample(st, logits, vocab, rows, keys, params, adv, sel, win, con);
        if (kind == kKindTop) { // [finish + top] in the place of [finish]: the merge launch only read the lists
            if (raw_select()) launch_sample_select(st, logits, vocab, rows, keys_raw); // (for all rows, so the launches stay uniform)
            launch_logprob_finish_top(st, logits, vocab, rows, part, raw_select() ? keys_raw : keys, top);
        } else if (kind == kKindLogprobs) {
            launch_logprob_finish(st, logits, vocab, rows, part, top.chosen); // (behind the advance: it knows whether a token was emitted)
        }
    }
};

// the loops' part of a tail over the program's blocks (after the ensure_* calls: the pointers are final); adv / win / top differ
SampledTail resident_tail(const Resident* r, uint32_t rows, SampledSel sel, SampledKind kind) {
    SampledTail t;
    t.rows = rows, t.sel = sel, t.kind = kind;
    t.keys = r->skeys, t.keys_raw = r->skeys_raw, t.params = r->sparams, t.part = r->lpart;
    t.con = constraint_args(r);
    t.top.params = r->sparams;
    return t;
}

// What the two batched loops ask of a request, refused before anything is enqueued: -> the steps of the call (the largest
// count) and the last position of every sequence. tokens_out (and n_produced) are filled only once nothing is refused.
// A sequence that stops before the last step repeats its step at the position BEHIND its last token (it rewrites that KV column
// with the same values): that column must exist too. (One frozen by a stop token idles at a position its own count covers.)
bool batch_request(zgml_hip_ctx* ctx, const Resident* r, const std::string& who, const uint32_t* first_tokens, const uint32_t* start_pos, const uint32_t* n_steps,
                   uint32_t max_steps, int64_t* tokens_out, uint32_t* n_produced, uint32_t* steps_out, std::vector<uint32_t>* last_pos) {
    const uint32_t B = r->n_seqs;
    uint32_t steps = 0;
    for (uint32_t b = 0; b < B; b++) steps = std::max(steps, n_steps[b]);
    if (steps > max_steps) {
        ctx->fail(who + ": n_steps exceeds max_steps");
        return false;
    }
    last_pos->resize(B);
    for (uint32_t b = 0; b < B; b++) {
        const uint64_t end = (uint64_t)start_pos[b] + n_steps[b]; // position after its last step
        const bool idles = n_steps[b] < steps;
        if (first_tokens[b] >= r->vocab || end > r->max_seq || (idles && end >= r->max_seq)) {
            ctx->fail(who + ": token or position out of range (sequence " + std::to_string(b) + ")");
            return false;
        }
        (*last_pos)[b] = (uint32_t)(idles ? end : (n_steps[b] ? end - 1 : start_pos[b]));
    }
    for (uint64_t i = 0; i < (uint64_t)B * max_steps; i++) tokens_out[i] = -1;
    for (uint32_t b = 0; n_produced && b < B; b++) n_produced[b] = 0;
    *steps_out = steps;
    return true;
}

// The flat index space of a prep launch (kernels.h): T embedding rows, T mask columns, T RoPE rows per layer leaf, the dynamic
// words — T the plan's token_len, which is B of a batched plan. The set-up refuses a plan whose total does not fit the
// launch's 32-bit argument and keeps the value: the op list's length is fixed when the program is created
// (zgml_hip_refresh_program refuses another), so the n_ops the argument structs read at every call is the one counted here
uint64_t prep_total(const Resident* r, size_t n_ops) {
    return (uint64_t)r->token_len * ((uint64_t)r->d + r->max_seq + (uint64_t)r->n_rope * 2 * r->dh) + n_ops;
}

// the prep launch of a single-sequence plan: position from state[1], the token_len token ids from `tokens`
struct Prep {
    ResidentPrepArgs a;
    uint32_t total;
};
Prep prep_args(const zgml_hip_program* p, const uint32_t* state, const uint32_t* tokens) {
    const Resident* r = p->resident;
    return {{r->embed, r->cos, r->sin, r->tok_in, r->mask, r->rope_bufs, r->dyn_kind, r->dyn_base, r->dyn_stride,
             p->dyn_dev, state, tokens, r->d, r->max_seq, r->dh, r->n_rope, (uint32_t)p->ops.size(), r->token_len},
            r->prep_total};
}

// ... and of a batched plan: everything from bstate
struct BatchPrep {
    ResidentBatchPrepArgs a;
    uint32_t total;
};
BatchPrep batch_prep_args(const zgml_hip_program* p) {
    const Resident* r = p->resident;
    return {{r->embed, r->cos, r->sin, r->tok_in, r->mask, r->rope_bufs, r->dyn_kind, r->dyn_base, r->dyn_stride, r->dyn_seq,
             p->dyn_dev, r->bstate, r->d, r->max_seq, r->dh, r->n_rope, (uint32_t)p->ops.size(), r->n_seqs},
            r->prep_total};
}

// A loop's step becomes a graph the first time it runs with graphs on (a failed capture leaves the slot empty: eager below).
// `wait`: host memory that a copy enqueued before this reads must not be in flight when the capture begins
template <class Step>
void capture_once(zgml_hip_ctx* ctx, hipStream_t s, const std::string& name, bool wait, Step step, GraphSlot& slot) {
    if (!ctx->opt_graph || slot.exec) return;
    if (wait) hipStreamSynchronize(s);
    capture_graph(ctx, s, name.c_str(), [&] { step(s); }, &slot);
}

// ... and runs n times: the graph, or the step's launches
template <class Step>
void replay(hipStream_t s, const GraphSlot& slot, uint32_t n, Step step) {
    for (uint32_t i = 0; i < n; i++) {
        if (slot.exec)
            hipGraphLaunch(slot.exec, s);
        else
            step(s);
    }
}

// The copy-out of a sampled loop's values and alternatives: download() enqueues the copies of the first `n` device entries
// (they lie as the produced tokens do); keep(), behind the synchronisation, leaves what the result getters hand out — `entries`
// values and [entries][width] pairs, entry e from device entry src(e), or the NaN / padding where src(e) < 0
struct SampledCopyOut {
    SampledKind kind;
    std::vector<float> lp, top_val;
    std::vector<uint32_t> top_tok;
    void download(hipStream_t s, const Resident* r, uint64_t n) {
        if (kind != kKindPick) {
            lp.resize(n);
            hipMemcpyAsync(lp.data(), r->lp, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s);
        }
        if (kind == kKindTop) {
            top_tok.resize((size_t)n * kTopLogprobsMax), top_val.resize(top_tok.size());
            hipMemcpyAsync(top_tok.data(), r->top_tok, top_tok.size() * 4, hipMemcpyDeviceToHost, s);
            hipMemcpyAsync(top_val.data(), r->top_val, top_val.size() * sizeof(float), hipMemcpyDeviceToHost, s);
        }
    }
    template <class LpSrc, class TopSrc>
    void keep(zgml_hip_ctx* ctx, uint64_t entries, uint32_t width, LpSrc lp_src, TopSrc top_src) const {
        if (kind != kKindPick) {
            ctx->lp_last.resize(entries);
            logprob_fill_unproduced(ctx->lp_last.data(), 0, entries);
            for (uint64_t e = 0; e < entries; e++)
                if (const int64_t from = lp_src(e); from >= 0) ctx->lp_last[e] = lp[(size_t)from];
        }
        if (kind == kKindTop) top_keep(ctx, entries, width, top_tok, top_val, top_src);
    }
};

} // namespace

extern "C" {

int zgml_hip_resident_setup(zgml_hip_ctx* ctx, zgml_hip_program* p, const zgml_resident_llama* d) {
    if (!ctx || !p || !d) return -1;
    hipSetDevice(ctx->device);
    free_resident(p);
    auto live = [&](uint16_t b) { return b < p->bufs.size() && p->bufs[b]; };
    if (!live(d->buf_token_input) || !live(d->buf_attn_mask) || !live(d->buf_logits) || !d->d_model ||
        p->sizes[d->buf_token_input] < d->d_model || p->sizes[d->buf_attn_mask] < d->max_seq ||
        p->sizes[d->buf_logits] < d->vocab) {
        ctx->fail("resident_setup: bad buffer ids");
        return -1;
    }
    // token_len of the plan: token_input holds T embedding rows (T = 1: decode plan, T > 1: prefill chunk)
    const uint32_t T = (uint32_t)(p->sizes[d->buf_token_input] / d->d_model);
    if (T > 1 && (p->sizes[d->buf_attn_mask] < (uint64_t)T * d->max_seq || p->sizes[d->buf_logits] < (uint64_t)T * d->vocab)) {
        ctx->fail("resident_setup: attn_mask / logits smaller than token_len columns / rows");
        return -1;
    }
    if (p->n_seqs && (T == 0 || T % p->n_seqs != 0)) {
        ctx->fail("resident_setup: the program declares " + std::to_string(p->n_seqs) + " sequences but token_input holds " + std::to_string(T) +
                  " columns (not a multiple of them)");
        return -1;
    }
    // built here and published only when everything has succeeded: every failure below leaves a program without a set-up
    std::unique_ptr<Resident> owner(new Resident());
    Resident* const r = owner.get();
    r->graph_epoch = ++g_graph_epoch;
    r->token_len = T;
    // > 0: the T columns are n_seqs sequences of tokens_per_seq consecutive positions each — one (zgml_hip_resident_decode_batch) or
    // several (zgml_hip_resident_decode_batch_speculative) —, not T consecutive positions of one
    r->n_seqs = p->n_seqs;
    r->tokens_per_seq = p->n_seqs ? T / p->n_seqs : 1;
    r->vocab = d->vocab, r->d = d->d_model, r->max_seq = d->max_seq, r->dh = d->d_head, r->n_rope = d->n_rope;
    r->tok_in = p->bufs[d->buf_token_input], r->mask = p->bufs[d->buf_attn_mask], r->logits = p->bufs[d->buf_logits];
    const size_t n_ops = p->ops.size();
    if (prep_total(r, n_ops) > UINT32_MAX) {
        ctx->fail("resident_setup: token_len x (d_model + max_seq + 2 n_rope d_head) + ops exceeds 2^32 - 1, the prep launch's index space");
        return -1;
    }
    r->prep_total = (uint32_t)prep_total(r, n_ops);
    std::vector<float*> ropes(d->n_rope);
    for (uint32_t l = 0; l < d->n_rope; l++) {
        if (!live(d->buf_rope[l]) || p->sizes[d->buf_rope[l]] < (uint64_t)T * 2 * d->d_head) {
            ctx->fail("resident_setup: bad rope buffer");
            return -1;
        }
        ropes[l] = p->bufs[d->buf_rope[l]];
    }
    std::vector<uint32_t> kind(n_ops, 0), base(n_ops, 0), stride(n_ops, 0);
    for (size_t i = 0; i < n_ops; i++) // the device's copy of dyn_field for the ops that move (the prep kernels evaluate DynField::at)
        if (const DynField f = dyn_field(p->ops[i]); f.moves()) kind[i] = f.role == DynField::SeqKv ? 2 : 1, base[i] = f.base, stride[i] = f.stride;
    const size_t tab = (size_t)d->max_seq * d->d_head, emb = (size_t)d->vocab * d->d_model; // elements
    bool ok = ensure_blocks(ctx, nullptr, r->embed, emb, r->cos, tab, r->sin, tab, r->rope_bufs, ropes.size() + 1, r->dyn_kind, n_ops + 1, r->dyn_base, n_ops + 1,
                            r->dyn_stride, n_ops + 1, r->state, 4, r->tok_dev, T) &&
              CTX_CHECK(ctx, h2d_sync(ctx->stream, r->embed, d->token_embed, emb * 4)) &&
              CTX_CHECK(ctx, h2d_sync(ctx->stream, r->cos, d->cos_table, tab * 4)) &&
              CTX_CHECK(ctx, h2d_sync(ctx->stream, r->sin, d->sin_table, tab * 4)) &&
              CTX_CHECK(ctx, h2d_sync(ctx->stream, r->rope_bufs, ropes.data(), ropes.size() * sizeof(float*))) &&
              CTX_CHECK(ctx, h2d_sync(ctx->stream, r->dyn_kind, kind.data(), n_ops * 4)) &&
              CTX_CHECK(ctx, h2d_sync(ctx->stream, r->dyn_base, base.data(), n_ops * 4)) &&
              CTX_CHECK(ctx, h2d_sync(ctx->stream, r->dyn_stride, stride.data(), n_ops * 4));
    if (ok && r->n_seqs) {
        std::vector<uint32_t> seq(n_ops + 1, 0);
        for (size_t i = 0; i < n_ops; i++) seq[i] = kind[i] && i < p->op_seq.size() && p->op_seq[i] != UINT32_MAX ? p->op_seq[i] : 0;
        const size_t pairs = (size_t)T * argmax_batch_blocks(d->vocab); // (a row per column: n_seqs, or n_seqs * tokens_per_seq of a verify step)
        ok = ensure_blocks(ctx, nullptr, r->bstate, (size_t)4 * r->n_seqs + 1, r->dyn_seq, n_ops + 1, r->bval, pairs, r->bidx, pairs) &&
             CTX_CHECK(ctx, h2d_sync(ctx->stream, r->dyn_seq, seq.data(), n_ops * 4));
    }
    if (!ok) return -1;
    p->resident = owner.release();
    // The resident kernels write token_input, attn_mask and the rope buffers from the device, outside the op list: to the hoist
    // analysis those buffers look like constants (never written by an op), so a `repeat` that broadcasts one of them would have
    // been run once at plan build and its stale copy read ever after. Today's LLaMA stream only repeats gamma and the
    // scalar 1, but the guard must not depend on that: every buffer handed over here leaves the hoisted set.
    unhoist_if_guarded(p, d->buf_token_input);
    unhoist_if_guarded(p, d->buf_attn_mask);
    for (uint32_t l = 0; l < d->n_rope; l++) unhoist_if_guarded(p, d->buf_rope[l]);
    return 0;
}

int zgml_hip_resident_decode(zgml_hip_ctx* ctx, zgml_hip_program* p, uint32_t first_token, uint32_t start_pos,
                             uint32_t n_steps, int64_t* tokens_out) {
    if (!ctx || !p || !p->resident || !tokens_out) return -1;
    Resident* r = p->resident;
    if (refuse_constrained(ctx, p, "resident_decode")) return -1;
    if (r->n_seqs) {
        ctx->fail("resident_decode: the program is a batched plan (sequences declared: use zgml_hip_resident_decode_batch)");
        return -1;
    }
    if (r->token_len != 1) {
        ctx->fail("resident_decode: the program is a token_len > 1 plan (use zgml_hip_resident_prefill)");
        return -1;
    }
    if (first_token >= r->vocab || (uint64_t)start_pos + n_steps > r->max_seq) {
        ctx->fail("resident_decode: token or position out of range");
        return -1;
    }
    hipSetDevice(ctx->device);
    hipStream_t s = ctx->stream;
    // the first and the last position of this call; a call of no steps probes nothing (there is no last position)
    resident_begin(p, [&] {
        return !n_steps || (positions_in_bounds(p, 1, [&](uint32_t) { return start_pos; }) && positions_in_bounds(p, 1, [&](uint32_t) { return start_pos + n_steps - 1; }));
    });
    if (!grow_tables(ctx, p, r->tokens, n_steps)) return -1;
    const Prep prep = prep_args(p, r->state, r->state /* the token is state[0] */);
    // Per token [plan] [stage 2 + advance + embedding row], one full prep in front of the call's first step. A step's patches
    // come from the step before it, through ordinary kernel boundaries: the launch that leaves the argmax pairs also writes the
    // position part of the next step's prep (it depends on the position alone, and nothing behind that launch reads those
    // buffers), and stage 2, which knows the token, copies its embedding row. The launch with the pairs is the tied LM head in
    // its streaming form, armed through run_plan with a block that exists for this call only (kernels.h: DenseHeadTail); where
    // the head is another kernel (a Q4_0 head) nothing takes the block up and the step is [plan] [stage 1 + position part]
    // [stage 2 + ...]. profiles/r18_token_tail.txt has the measurements.
    // (A token tail in ONE launch — the argmax, the advance of the device state and the next token's patches behind a
    // last-arriver count — was measured and removed. First form — the last arriver walks all 8-16 K elements of the next
    // token's patches alone — SLOWER: SmolLM-135M 1756 against 1773 tok/s, Llama-2-7B 790 against 817. Second form — every
    // workgroup writes the position-only patches, the last arriver the embedding row — a wash: 1777-1782 against 1768-1780, 838
    // against 842; profiles/r05_token_tail_ab.txt. The present form adds no synchronisation inside a launch.)
    const ArgmaxAdvance adv{r->state, r->tokens, r->tokens_cap(), r->embed, r->tok_in, r->d};
    DenseHeadTail head;
    head.logits = r->logits, head.vocab = r->vocab, head.pair_val = ctx->arg_val, head.pair_idx = ctx->arg_idx;
    head.ahead = ResidentAhead{prep.a, prep.total - r->token_len * r->d};
    auto one_token = [&](hipStream_t st) {
        head.pairs = 0;
        run_plan(p, st, 0, p->plan.size(), &head);
        if (head.pairs)
            launch_argmax_fold(st, ctx->arg_val, ctx->arg_idx, head.pairs, ctx->arg_out, adv);
        else
            launch_argmax(st, r->logits, r->vocab, ctx->arg_val, ctx->arg_idx, ctx->arg_out, adv, &head.ahead);
        r->tail_launches = head.pairs ? 1 : 2;
    };
    const uint32_t st0[4] = {first_token, start_pos, 0, 0}; // (a stack array: no wait before the capture, unlike the batched loop's vector)
    if (!CTX_CHECK(ctx, hipMemcpyAsync(r->state, st0, sizeof(st0), hipMemcpyHostToDevice, s))) return fail_after_copies(s);
    if (n_steps) launch_resident_prep(s, prep.a, prep.total); // the first step's patches, for (first_token, start_pos)
    capture_once(ctx, s, "resident", false, one_token, r->graph);
    // several tokens per graph launch: everything a token needs is produced on the device from the state words, so a graph may
    // simply hold the launches of G consecutive tokens (experiment: is there a per-graph gap on the device?)
    const uint32_t per_graph = (uint32_t)sw().hip_resident_tokens_per_graph;
    const auto tokens_of_a_graph = [&] {
        for (uint32_t t = 0; t < per_graph; t++) one_token(s);
    };
    if (ctx->opt_graph && r->graph.exec && per_graph > 1 && n_steps >= per_graph && !r->graph_multi.exec &&
        capture_graph(ctx, s, nullptr, tokens_of_a_graph, &r->graph_multi))
        r->multi_n = per_graph;
    for (uint32_t i = 0; i < n_steps;) {
        if (r->graph_multi.exec && n_steps - i >= r->multi_n) {
            hipGraphLaunch(r->graph_multi.exec, s);
            i += r->multi_n;
        } else if (r->graph.exec) {
            hipGraphLaunch(r->graph.exec, s);
            i++;
        } else {
            one_token(s);
            i++;
        }
    }
    hipMemcpyAsync(tokens_out, r->tokens, (size_t)n_steps * 8, hipMemcpyDeviceToHost, s);
    bool ok = CTX_CHECK(ctx, hipStreamSynchronize(s));
    ok = ok && ctx->handoff_ok("resident_decode");
    resident_end(p, n_steps, p->plan.size() + r->tail_launches); // per token [plan] [stage 2], or [plan] [argmax x 2]
    return ok ? 0 : -1;
}


// The resident loop over a batched program: per step [batched prep] [plan] [pick stage 1] [pick stage 2 + advance], one graph launch.
int zgml_hip_resident_decode_batch(zgml_hip_ctx* ctx, zgml_hip_program* p, const uint32_t* first_tokens, const uint32_t* start_pos,
                                   const uint32_t* n_steps, uint32_t max_steps, int64_t* tokens_out) {
    if (!ctx || !p) return -1;
    Resident* r = p->resident;
    if (!r || !r->n_seqs || !p->n_seqs) {
        ctx->fail("resident_decode_batch: not a batched program with a resident set-up (zgml_hip_program_set_sequences, then zgml_hip_resident_setup)");
        return -1;
    }
    if (refuse_verify_plan(ctx, r, "resident_decode_batch")) return -1;
    if (!first_tokens || !start_pos || !n_steps || (max_steps && !tokens_out)) return -1;
    if (refuse_constrained(ctx, p, "resident_decode_batch")) return -1;
    const uint32_t B = r->n_seqs;
    uint32_t steps = 0;
    std::vector<uint32_t> last_pos;
    if (!batch_request(ctx, r, "resident_decode_batch", first_tokens, start_pos, n_steps, max_steps, tokens_out, nullptr, &steps, &last_pos)) return -1;
    if (!steps) return 0;
    hipSetDevice(ctx->device);
    hipStream_t s = ctx->stream;
    // the first and the last position of every sequence
    resident_begin(p, [&] {
        return positions_in_bounds(p, 1, [&](uint32_t i) { return start_pos[p->op_seq[i]]; }) && positions_in_bounds(p, 1, [&](uint32_t i) { return last_pos[p->op_seq[i]]; });
    });
    if (!grow_tables(ctx, p, r->btokens, (size_t)B * steps)) return -1;
    const BatchPrep prep = batch_prep_args(p);
    auto one_step = [&](hipStream_t st) {
        launch_resident_batch_prep(st, prep.a, prep.total);
        run_plan(p, st, 0, p->plan.size());
        launch_argmax_batch(st, r->logits, r->vocab, B, r->bval, r->bidx, r->bstate, r->btokens);
    };
    std::vector<uint32_t> st0((size_t)4 * B + 1, 0);
    for (uint32_t b = 0; b < B; b++) st0[b] = first_tokens[b], st0[B + b] = start_pos[b], st0[2 * B + b] = n_steps[b];
    st0[4 * B] = steps; // row length of the device token table of this call
    if (!CTX_CHECK(ctx, hipMemcpyAsync(r->bstate, st0.data(), st0.size() * 4, hipMemcpyHostToDevice, s)) ||
        !CTX_CHECK(ctx, hipMemsetAsync(r->btokens, 0xFF, (size_t)B * steps * 8, s))) // (-1: what a sequence leaves behind its count)
        return fail_after_copies(s);
    // st0, a heap vector, is read by the copy above: it must not die under a pageable-memory copy in flight. (The
    // single-sequence loop hands over a 16-byte stack array instead and does without the wait.)
    capture_once(ctx, s, "resident_batch", true, one_step, r->graph);
    replay(s, r->graph, steps, one_step);
    std::vector<int64_t> got((size_t)B * steps);
    hipMemcpyAsync(got.data(), r->btokens, got.size() * 8, hipMemcpyDeviceToHost, s);
    bool ok = CTX_CHECK(ctx, hipStreamSynchronize(s));
    ok = ok && ctx->handoff_ok("resident_decode_batch");
    for (uint32_t b = 0; ok && b < B; b++)
        for (uint32_t i = 0; i < steps; i++) tokens_out[(uint64_t)b * max_steps + i] = got[(uint64_t)b * steps + i];
    resident_end(p, steps, p->plan.size() + 3); // per step [batched prep] [plan] [pick x 2]
    return ok ? 0 : -1;
}


// ── the sampled tail (contract: include/zgml_hip.h; rule: sample.h; kernels: sample.hip) ──

int64_t zgml_hip_sample(zgml_hip_ctx* ctx, zgml_hip_program* p, uint16_t buf_idx, uint64_t offset, uint64_t n, const zgml_sampling* sampling,
                        uint32_t position, uint32_t* candidates_out, uint32_t* n_candidates_out) {
    if (!ctx || !p) return -1;
    if (buf_idx >= p->bufs.size() || !p->bufs[buf_idx] || offset > p->sizes[buf_idx] || n > p->sizes[buf_idx] - offset || !n || n > 0xFFFFFFFFull) {
        ctx->fail("sample: the range must lie inside the buffer and hold 1 .. 2^32 - 1 elements");
        return -1;
    }
    SampleParamsDev sp;
    if (!sampling_params(ctx, "sample", sampling, 0, n, &sp)) return -1;
    hipSetDevice(ctx->device);
    hipStream_t s = ctx->stream;
    constexpr size_t out_words = 3 + kSampleMaxK;
    if (!ensure_blocks(ctx, nullptr, ctx->smp_keys, (size_t)kSampleMaxSlices * kSampleMaxK, ctx->smp_params, 1, ctx->smp_out, out_words)) return -1;
    if (sampling->logprobs && !ensure_ctx_logprob(ctx, 1)) return -1;
    const uint32_t top = sp.top_logprobs; // (0 without the `logprobs` word)
    if (top && !ensure_ctx_top(ctx, 1, sample_scratch_keys(n, 1))) return -1;
    if (sp.pen_active && !ensure_blocks(ctx, nullptr, ctx->smp_win, kSamplePenaltyMaxWindow)) return -1;
    if (!CTX_CHECK(ctx, hipMemcpyAsync(ctx->smp_params, &sp, sizeof(sp), hipMemcpyHostToDevice, s))) return fail_after_copies(s);
    // sequence 0's constraint, when the row is a row of the automaton's vocabulary: its state masks the pick and advances over it
    const Resident* const res = p->resident;
    const bool constrained = res && res->n_con && res->con[0] && n == res->vocab;
    SampledTail tail;
    tail.sel = SampledTail::sel_of(constrained, sp.pen_active), tail.kind = SampledTail::kind_of(sampling->logprobs, top);
    tail.keys = ctx->smp_keys, tail.keys_raw = ctx->top_keys, tail.params = ctx->smp_params, tail.part = ctx->lp_part;
    tail.adv.position = position, tail.adv.out = (int64_t*)ctx->smp_out.get(), tail.adv.cand = ctx->smp_out + 2;
    if (sp.pen_active) { // the window: the last W of the recent tokens, the token whose logits these are last
        const uint32_t take = std::min(sampling->n_recent, sp.window);
        if (take && !CTX_CHECK(ctx, hipMemcpyAsync(ctx->smp_win, sampling->recent + (sampling->n_recent - take), (size_t)take * 4, hipMemcpyHostToDevice, s))) return fail_after_copies(s);
        tail.win.list = ctx->smp_win, tail.win.n_list = take;
    }
    if (constrained) tail.con = constraint_args(res);
    // the values over the raw row, behind the pick: the token is read where the merge launch stored it
    tail.top.chosen.out = ctx->lp_out, tail.top.chosen.token64 = (const int64_t*)ctx->smp_out.get();
    tail.top.top_tok = ctx->top_tok, tail.top.top_val = ctx->top_val, tail.top.params = ctx->smp_params;
    tail.launch(s, p->bufs[buf_idx] + offset, n);
    float lp = 0.0f;
    std::vector<uint32_t> top_tok(top ? kTopLogprobsMax : 0);
    std::vector<float> top_val(top_tok.size());
    if (top) {
        hipMemcpyAsync(top_tok.data(), ctx->top_tok, kTopLogprobsMax * 4, hipMemcpyDeviceToHost, s);
        hipMemcpyAsync(top_val.data(), ctx->top_val, kTopLogprobsMax * sizeof(float), hipMemcpyDeviceToHost, s);
    }
    if (sampling->logprobs) hipMemcpyAsync(&lp, ctx->lp_out, sizeof(lp), hipMemcpyDeviceToHost, s);
    uint32_t got[out_words];
    hipMemcpyAsync(got, ctx->smp_out, sizeof(got), hipMemcpyDeviceToHost, s);
    if (!CTX_CHECK(ctx, hipStreamSynchronize(s)) || !ctx->handoff_ok("sample")) return -1;
    if (sampling->logprobs) ctx->lp_last.assign(1, lp);
    if (top) top_keep(ctx, 1, top_logprobs_count(top, n), top_tok, top_val, [](uint64_t) { return (int64_t)0; });
    const uint32_t kc = std::min<uint32_t>(got[2], kSampleMaxK);
    if (n_candidates_out) *n_candidates_out = kc;
    if (candidates_out) memcpy(candidates_out, got + 3, (size_t)kc * 4);
    int64_t token;
    memcpy(&token, got, 8);
    if (token < 0) ctx->fail("sample: the constraint's state allows no token");
    return token;
}

// ── the constraint (contract: include/zgml_hip.h; rule: sample.h; validation: sample_params.h) ──

zgml_hip_constraint* zgml_hip_constraint_create(zgml_hip_ctx* ctx, const zgml_token_dfa* dfa) {
    if (!ctx) return nullptr;
    if (const char* why = constraint_check(dfa)) {
        ctx->fail(std::string("constraint_create: ") + why);
        return nullptr;
    }
    hipSetDevice(ctx->device);
    zgml_hip_constraint* c = new zgml_hip_constraint();
    c->n_states = dfa->n_states, c->n_classes = dfa->n_classes, c->vocab = dfa->vocab;
    const size_t cls = (size_t)dfa->vocab * 2, nxt = (size_t)dfa->n_states * dfa->n_classes * 2, frc = (size_t)dfa->n_states * 4;
    // the forced token of every state, for the verify step under a constraint: once, beside the two tables
    std::vector<uint32_t> count(dfa->n_classes), first(dfa->n_classes), forced(dfa->n_states);
    constraint_forced(dfa, count.data(), first.data(), forced.data());
    if (!ensure_blocks(ctx, nullptr, c->class_of, cls / 2, c->next, nxt / 2, c->forced, frc / 4) ||
        !CTX_CHECK(ctx, h2d_sync(ctx->stream, c->class_of, dfa->class_of, cls)) || !CTX_CHECK(ctx, h2d_sync(ctx->stream, c->next, dfa->next, nxt)) ||
        !CTX_CHECK(ctx, h2d_sync(ctx->stream, c->forced, forced.data(), frc))) {
        delete c;
        return nullptr;
    }
    return c;
}

void zgml_hip_constraint_free(zgml_hip_ctx* ctx, zgml_hip_constraint* c) {
    if (!ctx || !c) return;
    if (c->attached) {
        ctx->fail("constraint_free: the constraint is still attached to " + std::to_string(c->attached) + " sequence(s) (detach it first)");
        return;
    }
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    delete c;
}

int zgml_hip_program_set_constraint(zgml_hip_ctx* ctx, zgml_hip_program* p, uint32_t seq, zgml_hip_constraint* c, uint32_t state) {
    if (!ctx || !p) return -1;
    Resident* r = p->resident;
    if (!r) {
        ctx->fail("program_set_constraint: the program has no resident set-up (zgml_hip_resident_setup first)");
        return -1;
    }
    const uint32_t rows = r->n_seqs ? r->n_seqs : 1;
    if (const char* why = constraint_attach_check(c ? c->vocab : r->vocab, c ? c->n_states : 1, r->vocab, rows, seq, c ? state : 0)) {
        ctx->fail(std::string("program_set_constraint: ") + why);
        return -1;
    }
    if (!c && (r->con.empty() || !r->con[seq])) return 0; // nothing attached, nothing to detach
    hipSetDevice(ctx->device);
    hipStream_t s = ctx->stream;
    const bool first = !r->con_rows;
    if (!ensure_row_blocks(ctx, p, "the constraint table", r->con_rows.count(), rows, r->con_rows, rows, r->con_state, rows) ||
        (first && !CTX_CHECK(ctx, hipMemsetAsync(r->con_state, 0, (size_t)rows * 4, s)))) // (on the stream of the uploads below: it is a non-blocking one, which a memset on the null stream is not ordered with)
        return -1;
    r->con.resize(rows, nullptr);
    if (r->con[seq]) r->con[seq]->attached -= 1, r->n_con -= 1;
    r->con[seq] = c;
    if (c) c->attached += 1, r->n_con += 1;
    // the table as the kernels read it, whole (the pointers never move: the graphs bake them, nothing is invalidated)
    std::vector<SampleConstraintRow> table(rows);
    for (uint32_t b = 0; b < rows; b++) {
        const zgml_hip_constraint* const cb = r->con[b];
        table[b] = cb ? SampleConstraintRow{cb->class_of, cb->next, cb->n_classes, 1, cb->forced} : SampleConstraintRow{nullptr, nullptr, 0, 0, nullptr};
    }
    const uint32_t st = c ? state : 0;
    const bool ok = CTX_CHECK(ctx, hipMemcpyAsync(r->con_rows, table.data(), table.size() * sizeof(SampleConstraintRow), hipMemcpyHostToDevice, s)) &&
                    CTX_CHECK(ctx, hipMemcpyAsync(r->con_state + seq, &st, 4, hipMemcpyHostToDevice, s)) && CTX_CHECK(ctx, hipStreamSynchronize(s));
    return ok ? 0 : fail_after_copies(s);
}

int64_t zgml_hip_program_constraint_state(zgml_hip_ctx* ctx, zgml_hip_program* p, uint32_t seq) {
    if (!ctx || !p || !p->resident) return -1;
    const Resident* r = p->resident;
    if (seq >= r->con.size() || !r->con[seq]) return -1;
    hipSetDevice(ctx->device);
    uint32_t st = 0;
    if (!CTX_CHECK(ctx, hipMemcpyAsync(&st, r->con_state + seq, 4, hipMemcpyDeviceToHost, ctx->stream)) || !CTX_CHECK(ctx, hipStreamSynchronize(ctx->stream))) return -1;
    return (int64_t)st;
}

// log softmax(row i)[tokens[i]] of `rows` consecutive rows: [partial] [finish], whatever the number of rows
int zgml_hip_logprobs(zgml_hip_ctx* ctx, zgml_hip_program* p, uint16_t buf_idx, uint64_t offset, uint64_t n, uint32_t rows, const uint32_t* tokens,
                      float* logprobs_out) {
    if (!ctx || !p) return -1;
    const uint64_t buf_size = buf_idx < p->bufs.size() && p->bufs[buf_idx] ? p->sizes[buf_idx] : 0;
    if (const char* why = logprobs_check(buf_size, offset, n, rows, tokens, logprobs_out)) {
        ctx->fail(std::string("logprobs: ") + why);
        return -1;
    }
    hipSetDevice(ctx->device);
    hipStream_t s = ctx->stream;
    constexpr uint32_t kMaxGridRows = 4096; // rows per pair of launches: the block pairs of that many rows are 8 MiB (a grid's y extent is 65535)
    if (!ensure_ctx_logprob(ctx, std::min(rows, kMaxGridRows))) return -1;
    for (uint32_t r0 = 0; r0 < rows; r0 += kMaxGridRows) {
        const uint32_t nr = std::min(rows - r0, kMaxGridRows);
        const float* v = p->bufs[buf_idx] + offset + (uint64_t)r0 * n;
        if (!CTX_CHECK(ctx, hipMemcpyAsync(ctx->lp_tok, tokens + r0, (size_t)nr * 4, hipMemcpyHostToDevice, s))) return -1;
        LogprobTarget lt;
        lt.out = ctx->lp_out, lt.tokens = ctx->lp_tok;
        launch_logprob(s, v, n, nr, ctx->lp_part);
        launch_logprob_finish(s, v, n, nr, ctx->lp_part, lt);
        hipMemcpyAsync(logprobs_out + r0, ctx->lp_out, (size_t)nr * sizeof(float), hipMemcpyDeviceToHost, s);
        if (!CTX_CHECK(ctx, hipStreamSynchronize(s))) return -1; // (the caller's arrays are pageable memory: nothing of them in flight on return)
    }
    return ctx->handoff_ok("logprobs") ? 0 : -1;
}

// the min(top_n, n) largest logits of `rows` consecutive rows with their log-probabilities: [partial] [select] [finish + top]
int zgml_hip_top_logprobs(zgml_hip_ctx* ctx, zgml_hip_program* p, uint16_t buf_idx, uint64_t offset, uint64_t n, uint32_t rows, uint32_t top_n,
                          int64_t* tokens_out, float* logprobs_out) {
    if (!ctx || !p) return -1;
    const uint64_t buf_size = buf_idx < p->bufs.size() && p->bufs[buf_idx] ? p->sizes[buf_idx] : 0;
    if (const char* why = top_logprobs_check(buf_size, offset, n, rows, top_n, tokens_out, logprobs_out)) {
        ctx->fail(std::string("top_logprobs: ") + why);
        return -1;
    }
    hipSetDevice(ctx->device);
    hipStream_t s = ctx->stream;
    constexpr uint32_t kMaxGridRows = 1024; // rows per triple of launches: the lists of that many rows are at most 64 MiB
    const uint32_t chunk = std::min(rows, kMaxGridRows);
    if (!ensure_ctx_logprob(ctx, chunk) || !ensure_ctx_top(ctx, chunk, sample_scratch_keys(n, chunk))) return -1;
    std::vector<uint32_t> tok((size_t)chunk * kTopLogprobsMax);
    std::vector<float> val((size_t)chunk * kTopLogprobsMax);
    for (uint32_t r0 = 0; r0 < rows; r0 += kMaxGridRows) {
        const uint32_t nr = std::min(rows - r0, kMaxGridRows);
        const float* v = p->bufs[buf_idx] + offset + (uint64_t)r0 * n;
        TopLogprobTarget tt; // (no chosen token: the entry is the row)
        tt.top_tok = ctx->top_tok, tt.top_val = ctx->top_val, tt.top_n = top_n;
        launch_logprob(s, v, n, nr, ctx->lp_part);
        launch_sample_select(s, v, n, nr, ctx->top_keys);
        launch_logprob_finish_top(s, v, n, nr, ctx->lp_part, ctx->top_keys, tt);
        hipMemcpyAsync(tok.data(), ctx->top_tok, (size_t)nr * kTopLogprobsMax * 4, hipMemcpyDeviceToHost, s);
        hipMemcpyAsync(val.data(), ctx->top_val, (size_t)nr * kTopLogprobsMax * sizeof(float), hipMemcpyDeviceToHost, s);
        if (!CTX_CHECK(ctx, hipStreamSynchronize(s))) return -1;
        for (uint32_t i = 0; i < nr; i++)
            for (uint32_t j = 0; j < top_n; j++) { // (behind min(top_n, n) the kernel left 0xFFFFFFFF and the NaN)
                const uint32_t t = tok[(size_t)i * kTopLogprobsMax + j];
                tokens_out[(uint64_t)(r0 + i) * top_n + j] = t == 0xFFFFFFFFu ? -1 : (int64_t)t;
                logprobs_out[(uint64_t)(r0 + i) * top_n + j] = val[(size_t)i * kTopLogprobsMax + j];
            }
    }
    return ctx->handoff_ok("top_logprobs") ? 0 : -1;
}

// the alternatives the context's last call with `logprobs` and `top_logprobs` set left behind: [entries][width]
int64_t zgml_hip_top_logprobs_result(zgml_hip_ctx* ctx, int64_t* tokens_out, float* logprobs_out, uint64_t n, uint32_t* width_out) {
    if (!ctx) return -1;
    if ((!tokens_out || !logprobs_out) && n) {
        ctx->fail("top_logprobs_result: tokens_out and logprobs_out must not be NULL");
        return -1;
    }
    const uint64_t have = ctx->top_tok_last.size();
    if (const uint64_t take = std::min(n, have)) {
        memcpy(tokens_out, ctx->top_tok_last.data(), take * sizeof(int64_t));
        memcpy(logprobs_out, ctx->top_val_last.data(), take * sizeof(float));
    }
    if (width_out) *width_out = ctx->top_width_last;
    return (int64_t)have;
}

// the values the context's last call with the `logprobs` word set left behind, in the layout of that call's tokens_out
int64_t zgml_hip_logprobs_result(zgml_hip_ctx* ctx, float* out, uint64_t n) {
    if (!ctx) return -1;
    if (!out && n) {
        ctx->fail("logprobs_result: out must not be NULL");
        return -1;
    }
    const uint64_t have = ctx->lp_last.size();
    if (const uint64_t take = std::min(n, have)) memcpy(out, ctx->lp_last.data(), take * sizeof(float));
    return (int64_t)have;
}

// zgml_hip_resident_decode with [select] [merge + pick + advance] in the place of the two argmax stages
int zgml_hip_resident_decode_sampled(zgml_hip_ctx* ctx, zgml_hip_program* p, uint32_t first_token, uint32_t start_pos, uint32_t n_steps,
                                     const zgml_sampling* sampling, int64_t* tokens_out, uint32_t* n_produced) {
    if (!ctx || !p || !p->resident || (n_steps && !tokens_out)) return -1;
    Resident* r = p->resident;
    if (n_produced) *n_produced = 0;
    if (r->n_seqs) {
        ctx->fail("resident_decode_sampled: the program is a batched plan (sequences declared: use zgml_hip_resident_decode_batch_sampled)");
        return -1;
    }
    if (r->token_len != 1) {
        ctx->fail("resident_decode_sampled: the program is a token_len > 1 plan");
        return -1;
    }
    SampleParamsDev sp;
    if (!sampling_params(ctx, "resident_decode_sampled", sampling, r->vocab, r->vocab, &sp, RecentOf::Loop, start_pos)) return -1;
    if (first_token >= r->vocab || (uint64_t)start_pos + n_steps > r->max_seq) {
        ctx->fail("resident_decode_sampled: token or position out of range");
        return -1;
    }
    if (!n_steps) return 0;
    hipSetDevice(ctx->device);
    hipStream_t s = ctx->stream;
    resident_begin(p, [&] {
        return positions_in_bounds(p, 1, [&](uint32_t) { return start_pos; }) && positions_in_bounds(p, 1, [&](uint32_t) { return start_pos + n_steps - 1; });
    });
    const bool penalized = sp.pen_active != 0, lp = sampling->logprobs != 0, top = sp.top_logprobs != 0; // (top: only with lp)
    // a constraint attached: the constrained select launch, which serves penalties on and off (its graph bakes the window block)
    const bool constrained = r->n_con != 0;
    if (!ensure_sample_blocks(ctx, p, 1) || ((penalized || constrained) && !ensure_window_block(ctx, p, 1))) return -1;
    if (!grow_tables(ctx, p, r->tokens, n_steps)) return -1;
    if (lp && !ensure_logprob_blocks(ctx, p, 1, r->tokens)) return -1;
    if (top && !ensure_top_blocks(ctx, p, 1, r->tokens)) return -1;
    const Prep prep = prep_args(p, r->state, r->state /* the token is state[0] */);
    SampledTail tail = resident_tail(r, 1, SampledTail::sel_of(constrained, penalized), SampledTail::kind_of(lp, top));
    tail.adv.state = r->state, tail.adv.tokens = r->tokens, tail.adv.cap = r->tokens_cap();
    tail.win.ring = r->swin, tail.win.lo = r->swin + kSamplePenaltyMaxWindow;
    LogprobTarget& lt = tail.top.chosen;
    lt.out = r->lp, lt.state = r->state, lt.emitted = r->tokens, lt.written = r->lp_written, lt.cap = r->tokens_cap();
    tail.top.top_tok = r->top_tok, tail.top.top_val = r->top_val;
    auto one_token = [&](hipStream_t st) {
        launch_resident_prep(st, prep.a, prep.total);
        run_plan(p, st, 0, p->plan.size());
        tail.launch(st, r->logits, r->vocab);
    };
    std::vector<uint32_t> win0; // (penalised calls only; alive until the call's last synchronisation)
    if (penalized) {
        win0.assign(kSamplePenaltyMaxWindow + 1, 0);
        fill_window_block(win0, 1, 0, *sampling, start_pos);
        if (!CTX_CHECK(ctx, hipMemcpyAsync(r->swin, win0.data(), win0.size() * 4, hipMemcpyHostToDevice, s))) return fail_after_copies(s);
    }
    const uint32_t st0[4] = {first_token, start_pos, 0, 0}; // ([3]: set by a stop token)
    if (!CTX_CHECK(ctx, hipMemcpyAsync(r->state, st0, sizeof(st0), hipMemcpyHostToDevice, s)) ||
        !CTX_CHECK(ctx, hipMemcpyAsync(r->sparams, &sp, sizeof(sp), hipMemcpyHostToDevice, s)) ||
        !CTX_CHECK(ctx, hipMemsetAsync(r->tokens, 0xFF, (size_t)n_steps * 8, s)) || // (-1: what a stopped sequence leaves behind its stop token)
        (lp && !CTX_CHECK(ctx, hipMemsetAsync(r->lp_written, 0, 4, s))))
        return fail_after_copies(s);
    // (a penalised call replays a graph of its own, and so do a constrained call and a call with log-probabilities: the kinds of
    // call alternate on one program and invalidate nothing)
    GraphSlot& slot = r->sgraph[tail.form()];
    // (the copies above read this stack frame: none in flight when the capture begins)
    capture_once(ctx, s, std::string("resident_") + kSampledFormNames[tail.form()], true, one_token, slot);
    replay(s, slot, n_steps, one_token);
    uint32_t st1[4] = {0, 0, 0, 0};
    hipMemcpyAsync(tokens_out, r->tokens, (size_t)n_steps * 8, hipMemcpyDeviceToHost, s);
    hipMemcpyAsync(st1, r->state, sizeof(st1), hipMemcpyDeviceToHost, s);
    SampledCopyOut out{tail.kind};
    out.download(s, r, n_steps);
    bool ok = CTX_CHECK(ctx, hipStreamSynchronize(s));
    ok = ok && ctx->handoff_ok("resident_decode_sampled");
    const uint32_t made = ok ? std::min(st1[2], n_steps) : 0;
    if (ok && n_produced) *n_produced = made;
    const auto produced = [&](uint64_t e) { return e < made ? (int64_t)e : -1; };
    out.keep(ctx, n_steps, top_logprobs_count(sp.top_logprobs, r->vocab), produced, produced);
    // per token [prep] [plan] and the sampled tail
    resident_end(p, n_steps, p->plan.size() + 1 + tail.launches());
    return ok ? 0 : -1;
}

// zgml_hip_resident_decode_batch with the sampled tail, blockIdx.y = sequence in both of its launches
int zgml_hip_resident_decode_batch_sampled(zgml_hip_ctx* ctx, zgml_hip_program* p, const uint32_t* first_tokens, const uint32_t* start_pos,
                                           const uint32_t* n_steps, uint32_t max_steps, const zgml_sampling* per_seq, int64_t* tokens_out,
                                           uint32_t* n_produced) {
    if (!ctx || !p) return -1;
    Resident* r = p->resident;
    if (!r || !r->n_seqs || !p->n_seqs) {
        ctx->fail("resident_decode_batch_sampled: not a batched program with a resident set-up (zgml_hip_program_set_sequences, then zgml_hip_resident_setup)");
        return -1;
    }
    if (refuse_verify_plan(ctx, r, "resident_decode_batch_sampled")) return -1;
    if (!first_tokens || !start_pos || !n_steps || (max_steps && !tokens_out)) return -1;
    const uint32_t B = r->n_seqs;
    std::vector<SampleParamsDev> sp(B);
    for (uint32_t b = 0; b < B; b++)
        if (!sampling_params(ctx, "resident_decode_batch_sampled (sequence " + std::to_string(b) + ")", per_seq ? per_seq + b : nullptr, r->vocab, r->vocab, &sp[b], RecentOf::Loop, start_pos[b])) return -1;
    uint32_t steps = 0;
    std::vector<uint32_t> last_pos;
    if (!batch_request(ctx, r, "resident_decode_batch_sampled", first_tokens, start_pos, n_steps, max_steps, tokens_out, n_produced, &steps, &last_pos)) return -1;
    if (!steps) return 0;
    hipSetDevice(ctx->device);
    hipStream_t s = ctx->stream;
    resident_begin(p, [&] {
        return positions_in_bounds(p, 1, [&](uint32_t i) { return start_pos[p->op_seq[i]]; }) && positions_in_bounds(p, 1, [&](uint32_t i) { return last_pos[p->op_seq[i]]; });
    });
    bool penalized = false; // one sequence with penalties: the penalised launch for all (a row without them computes what it did)
    bool lp = false; // ... and one with log-probabilities: the two launches for all (a row nobody asked for is not copied out)
    bool top = false; // ... and one with alternatives: the top form of the finish for all (a row with the count 0 is all padding)
    for (uint32_t b = 0; b < B; b++) penalized = penalized || sp[b].pen_active, lp = lp || per_seq[b].logprobs, top = top || sp[b].top_logprobs;
    const bool constrained = r->n_con != 0; // one sequence with a constraint: the constrained launch for all (a row without one computes what it did)
    if (!ensure_sample_blocks(ctx, p, B) || ((penalized || constrained) && !ensure_window_block(ctx, p, B))) return -1;
    if (!grow_tables(ctx, p, r->btokens, (size_t)B * steps)) return -1;
    if (lp && !ensure_logprob_blocks(ctx, p, B, r->btokens)) return -1;
    if (top && !ensure_top_blocks(ctx, p, B, r->btokens)) return -1;
    const BatchPrep prep = batch_prep_args(p);
    SampledTail tail = resident_tail(r, B, SampledTail::sel_of(constrained, penalized), SampledTail::kind_of(lp, top));
    tail.adv.state = r->bstate, tail.adv.tokens = r->btokens, tail.adv.n_seqs = B;
    tail.win.ring = r->swin, tail.win.lo = r->swin + (size_t)B * kSamplePenaltyMaxWindow;
    LogprobTarget& lt = tail.top.chosen; // the values lie as the tokens do, [B][steps], and the pairs as the values
    lt.out = r->lp, lt.state = r->bstate, lt.emitted = r->btokens, lt.written = r->lp_written, lt.n_seqs = B;
    tail.top.top_tok = r->top_tok, tail.top.top_val = r->top_val;
    auto one_step = [&](hipStream_t st) {
        launch_resident_batch_prep(st, prep.a, prep.total);
        run_plan(p, st, 0, p->plan.size());
        tail.launch(st, r->logits, r->vocab);
    };
    std::vector<uint32_t> win0;
    if (penalized) {
        win0.assign((size_t)B * (kSamplePenaltyMaxWindow + 1), 0);
        for (uint32_t b = 0; b < B; b++) fill_window_block(win0, B, b, per_seq[b], start_pos[b]);
        if (!CTX_CHECK(ctx, hipMemcpyAsync(r->swin, win0.data(), win0.size() * 4, hipMemcpyHostToDevice, s))) return fail_after_copies(s);
    }
    std::vector<uint32_t> st0((size_t)4 * B + 1, 0), st1((size_t)4 * B + 1, 0);
    for (uint32_t b = 0; b < B; b++) st0[b] = first_tokens[b], st0[B + b] = start_pos[b], st0[2 * B + b] = n_steps[b];
    st0[4 * B] = steps; // row length of the device token table of this call
    if (!CTX_CHECK(ctx, hipMemcpyAsync(r->bstate, st0.data(), st0.size() * 4, hipMemcpyHostToDevice, s)) ||
        !CTX_CHECK(ctx, hipMemcpyAsync(r->sparams, sp.data(), sp.size() * sizeof(SampleParamsDev), hipMemcpyHostToDevice, s)) ||
        !CTX_CHECK(ctx, hipMemsetAsync(r->btokens, 0xFF, (size_t)B * steps * 8, s)) || // (-1: what a sequence leaves behind its count)
        (lp && !CTX_CHECK(ctx, hipMemsetAsync(r->lp_written, 0, (size_t)B * 4, s))))
        return fail_after_copies(s);
    GraphSlot& slot = r->sgraph[tail.form()];
    // (as the greedy batched loop: no pageable copy in flight when the capture begins)
    capture_once(ctx, s, std::string("resident_batch_") + kSampledFormNames[tail.form()], true, one_step, slot);
    replay(s, slot, steps, one_step);
    std::vector<int64_t> got((size_t)B * steps);
    hipMemcpyAsync(got.data(), r->btokens, got.size() * 8, hipMemcpyDeviceToHost, s);
    hipMemcpyAsync(st1.data(), r->bstate, st1.size() * 4, hipMemcpyDeviceToHost, s);
    SampledCopyOut out{tail.kind};
    out.download(s, r, (uint64_t)B * steps);
    bool ok = CTX_CHECK(ctx, hipStreamSynchronize(s));
    ok = ok && ctx->handoff_ok("resident_decode_batch_sampled");
    for (uint32_t b = 0; ok && b < B; b++) {
        for (uint32_t i = 0; i < steps; i++) tokens_out[(uint64_t)b * max_steps + i] = got[(uint64_t)b * steps + i];
        if (n_produced) n_produced[b] = std::min(st1[3 * B + b], n_steps[b]);
    }
    // [n_seqs][max_steps] values, as tokens_out, and [n_seqs][max_steps][width] pairs: the largest count among the sequences; a
    // sequence with a smaller one, or none, is padded, and one that did not ask keeps the NaN
    uint32_t width = 0;
    for (uint32_t b = 0; b < B; b++) width = std::max(width, top_logprobs_count(sp[b].top_logprobs, r->vocab));
    const auto produced = [&](uint64_t e, bool asked) {
        const uint32_t b = (uint32_t)(e / max_steps), i = (uint32_t)(e % max_steps);
        const uint32_t made = ok ? std::min(st1[3 * B + b], n_steps[b]) : 0;
        return asked && i < made ? (int64_t)((uint64_t)b * steps + i) : -1;
    };
    out.keep(ctx, (uint64_t)B * max_steps, width, [&](uint64_t e) { return produced(e, per_seq[e / max_steps].logprobs); },
             [&](uint64_t e) { return produced(e, sp[e / max_steps].top_logprobs); });
    // per step [batched prep] [plan] and the sampled tail
    resident_end(p, steps, p->plan.size() + 1 + tail.launches());
    return ok ? 0 : -1;
}


// One execution of a token_len = T plan (a prefill chunk) with everything but the T token ids produced on the device.
int64_t zgml_hip_resident_prefill(zgml_hip_ctx* ctx, zgml_hip_program* p, const uint32_t* tokens, uint32_t n_tokens, uint32_t start_pos) {
    if (!ctx || !p || !p->resident || !tokens) return -1;
    Resident* r = p->resident;
    if (r->n_seqs) {
        ctx->fail("resident_prefill: the program is a batched plan (sequences declared: use zgml_hip_resident_decode_batch)");
        return -1;
    }
    if (n_tokens != r->token_len || (uint64_t)start_pos + n_tokens > r->max_seq) {
        ctx->fail("resident_prefill: n_tokens must equal the plan's token_len and the chunk must fit max_seq");
        return -1;
    }
    for (uint32_t j = 0; j < n_tokens; j++)
        if (tokens[j] >= r->vocab) {
            ctx->fail("resident_prefill: token out of range");
            return -1;
        }
    hipSetDevice(ctx->device);
    hipStream_t s = ctx->stream;
    resident_begin(p, [&] { return positions_in_bounds(p, n_tokens, [&](uint32_t) { return start_pos; }); }); // (one execution: one position)
    const uint32_t st0[4] = {0, start_pos, 0, 0};
    if (!CTX_CHECK(ctx, hipMemcpyAsync(r->state, st0, sizeof(st0), hipMemcpyHostToDevice, s)) ||
        !CTX_CHECK(ctx, hipMemcpyAsync(r->tok_dev, tokens, (size_t)n_tokens * 4, hipMemcpyHostToDevice, s)))
        return fail_after_copies(s);
    const Prep prep = prep_args(p, r->state, r->tok_dev);
    launch_resident_prep(s, prep.a, prep.total);
    // through enqueue, not run_plan: one execution per call, so the program's own graphs (captured once, shared with
    // execute_program) are what to replay. dyn_dirty is cleared first: the prep launch has just written the device words, and
    // enqueue's flush_dyn must be a no-op rather than overwrite them with the host mirror
    p->dyn_dirty = false;
    enqueue(p);
    // the logits buffer holds one row per token: the greedy token comes from the LAST position's row
    launch_argmax(s, r->logits + (uint64_t)(n_tokens - 1) * r->vocab, r->vocab, ctx->arg_val, ctx->arg_idx, ctx->arg_out);
    hipMemcpyAsync(ctx->arg_out_host, ctx->arg_out, sizeof(int64_t), hipMemcpyDeviceToHost, s);
    const bool ok = CTX_CHECK(ctx, hipStreamSynchronize(s)) && ctx->handoff_ok("resident_prefill");
    resident_end(p, 1, p->plan.size() + 3); // [prep] [plan] [argmax x 2]
    return ok ? *ctx->arg_out_host : -1;
}


} // extern "C"

namespace {

// What the speculative loops ask of ONE sequence's request (include/zgml_hip.h), refused before anything is enqueued; -> the
// options with their defaults filled in. T: the columns of a verify step of the sequence. idle_at_end: the batched loop, whose
// finished sequences idle at their end position and store T columns there
struct SpecRequest {
    zgml_spec_decode o{nullptr, 0, 0, nullptr, 0, 0};
    uint32_t ngram = kSpecDefaultNgram, n_drafts = 0;
};
bool spec_request(zgml_hip_ctx* ctx, const Resident* r, const std::string& who, uint32_t first_token, uint32_t start_pos, uint32_t n_tokens, uint32_t T,
                  bool idle_at_end, const zgml_spec_decode* opt, SpecRequest* out) {
    if (opt) out->o = *opt;
    const zgml_spec_decode& o = out->o;
    out->ngram = o.ngram ? o.ngram : kSpecDefaultNgram;
    if (o.mode > 1 || out->ngram > kSpecMaxNgram) {
        ctx->fail(who + ": mode must be 0 or 1 and ngram at most " + std::to_string(kSpecMaxNgram));
        return false;
    }
    if ((o.n_history != 0 && o.n_history != start_pos) || (o.n_history && !o.history) || (o.mode == 1 && o.n_drafts && !o.drafts)) {
        ctx->fail(who + ": n_history must be 0 or start_pos (with the tokens), provided drafts need their array");
        return false;
    }
    // the last step may start at start_pos + n_tokens - 1 and stores T columns; an idle step starts one column behind that
    if ((uint64_t)start_pos + n_tokens + T - (idle_at_end ? 0 : 1) > r->max_seq) {
        ctx->fail(who + (idle_at_end ? ": start_pos + n_tokens + tokens_per_seq exceeds max_seq" : ": start_pos + n_tokens + token_len - 1 exceeds max_seq"));
        return false;
    }
    out->n_drafts = o.mode == 1 ? o.n_drafts : 0;
    bool in_vocab = first_token < r->vocab;
    for (uint32_t i = 0; in_vocab && i < o.n_history; i++) in_vocab = o.history[i] < r->vocab;
    for (uint32_t i = 0; in_vocab && i < out->n_drafts; i++) in_vocab = o.drafts[i] < r->vocab;
    if (!in_vocab) {
        ctx->fail(who + ": token out of range (first token, history or drafts)");
        return false;
    }
    return true;
}

// Speculative decode of one sequence over a token_len = T plan (contract: include/zgml_hip.h; rules: spec.h), both forms. Per
// verify step [draft] [prep, T tokens] [plan] [argmax stage 1 over T rows] [accept + advance], captured once as one graph; the
// sampled form (`sampled`: zgml_hip_resident_decode_speculative_sampled) has [select] [merge + pick] over the T rows in the
// place of the argmax stage — one launch more —, a graph of its own in the slot resident_decode_sampled cannot use on such a plan,
// and a stop token may end the call early. Everything the greedy form does is what it did before the sampled one existed.
// `honours_constraint` (zgml_hip_resident_decode_speculative_constrained; spec.h: UNDER A CONSTRAINT): the sampled form, and with
// a constraint attached to sequence 0 the constrained one — the same launches with the constrained-rows select in the place of
// the select, the draft and the accept launch also walking the automaton, graphs of their own; a reached state without a token
// ends the call early as a stop token does. Without a constraint it is the sampled form to the launch.
// `model` (zgml_hip_resident_decode_speculative_model; spec.h: DRAFTS FROM A MODEL): the candidates come from `draft`, a plain
// token_len = 1 program of the same context and vocabulary, executed T times between the draft launch and the prep —
//   [begin] T x { [draft prep] [draft plan] [argmax stage 1] [stage 2 + draft advance] } [prep] [plan] ... [accept]
// one graph launch, a linear chain. Either form of the verify step; `opt` carries the history alone. The graphs belong to the
// pair (Resident::pair_graph); each program's profile counts its own launches. The draft executions are the plain form: the
// streaming head and the position part written a token ahead (zgml_hip_resident_decode) are not carried over.
// `model` and `honours_constraint` (zgml_hip_resident_decode_speculative_model_constrained; spec.h: DRAFTS FROM A MODEL UNDER A
// CONSTRAINT): with a constraint attached to the target the two argmax launches of every draft execution are the masked ones
// (launch_argmax_draft_constrained) — execution j reads row j's state and writes row j + 1's — in front of the constrained verify
// step; launch for launch the chain above, in the pair's constrained-rows slots. Without a constraint it is the `model` form.
int spec_decode(zgml_hip_ctx* ctx, zgml_hip_program* p, const std::string& who, uint32_t first_token, uint32_t start_pos, uint32_t n_tokens,
                const zgml_spec_decode* opt, bool sampled, const zgml_sampling* sampling, int64_t* tokens_out, uint32_t* n_produced, zgml_spec_stats* stats,
                bool honours_constraint = false, bool model = false, zgml_hip_program* draft = nullptr) {
    if (!ctx || !p || !p->resident) return -1;
    Resident* r = p->resident;
    if (n_produced) *n_produced = 0;
    if (!honours_constraint && refuse_constrained(ctx, p, who.c_str())) return -1;
    if (model && !p->shard_points.empty()) {
        ctx->fail(who + ": the target is a sharded program (gather points attached)");
        return -1;
    }
    const bool constrained = honours_constraint && r->n_con != 0;
    if (r->n_seqs) {
        ctx->fail(who + ": the program is a batched plan (one sequence only here: zgml_hip_resident_decode_batch_speculative runs a batched plan with tokens_per_seq >= 2)");
        return -1;
    }
    const uint32_t T = r->token_len;
    if (T < 2) {
        ctx->fail(who + ": the program is a token_len = 1 plan (a verify step needs token_len >= 2)");
        return -1;
    }
    if (stats) *stats = zgml_spec_stats{0, 0, 0, 0};
    Resident* const dr = model && draft ? draft->resident : nullptr;
    if (model) { // what the call asks of the draft program
        const char* why = !draft ? "no draft program" : draft == p ? "the draft is the target program itself" : draft->ctx != p->ctx ? "the draft belongs to another context"
                          : !dr ? "the draft has no resident set-up (zgml_hip_resident_setup first)"
                          : dr->n_seqs ? "the draft is a batched plan" : dr->token_len != 1 ? "the draft must be a token_len = 1 plan"
                          : !draft->shard_points.empty() ? "the draft is a sharded program (gather points attached)"
                          : dr->vocab != r->vocab ? "the draft has another vocabulary than the target" : nullptr;
        if (why) {
            ctx->fail(who + ": " + why);
            return -1;
        }
        if (has_constraint(draft)) { // (the automaton that masks the drafts is the TARGET's: zgml_hip_resident_decode_speculative_model_constrained)
            ctx->fail(who + ": a constraint is attached to the draft program (detach it first)");
            return -1;
        }
    }
    if (!n_tokens) return 0;
    if (!tokens_out) return -1;
    SpecRequest req;
    if (!spec_request(ctx, r, who, first_token, start_pos, n_tokens, T, false, opt, &req)) return -1;
    if (dr && (uint64_t)start_pos + n_tokens + T - 1 > dr->max_seq) { // (the target's bound: the draft stores the same T columns per step)
        ctx->fail(who + ": start_pos + n_tokens + token_len - 1 exceeds the draft's max_seq");
        return -1;
    }
    const zgml_spec_decode& o = req.o;
    const uint32_t ngram = req.ngram, n_drafts = req.n_drafts;
    SampleParamsDev sp{};
    if (sampled && !sampling_params(ctx, who, sampling, r->vocab, r->vocab, &sp, RecentOf::Spec)) return -1;
    const bool penalized = sp.pen_active != 0, lp = sampled && sampling->logprobs, top = sp.top_logprobs != 0; // (sampled form only; top: only with lp)
    hipSetDevice(ctx->device);
    hipStream_t s = ctx->stream;
    // the first start and the last possible start of a verify step
    resident_begin(p, [&] {
        return positions_in_bounds(p, T, [&](uint32_t) { return start_pos; }) && positions_in_bounds(p, T, [&](uint32_t) { return start_pos + n_tokens - 1; });
    });
    // ... and the first and the last possible position of a draft execution
    if (dr) resident_begin(draft, [&] {
        return positions_in_bounds(draft, 1, [&](uint32_t) { return start_pos; }) && positions_in_bounds(draft, 1, [&](uint32_t) { return start_pos + n_tokens + T - 2; });
    });
    const uint32_t nblk = (uint32_t)argmax_batch_blocks(r->vocab), hist_cap = r->max_seq + 1;
    if (!ensure_row_blocks(ctx, p, "the verify step's blocks", r->bval.count() / nblk, T, r->spec, kSpecWords, r->hist, hist_cap, r->drafts, r->max_seq,
                           r->bval, (size_t)T * nblk, r->bidx, (size_t)T * nblk))
        return -1;
    if (sampled && (!ensure_sample_blocks(ctx, p, T) || !ensure_row_blocks(ctx, p, "the rows' picks", r->picks.count(), T, r->picks, T))) return -1;
    if (constrained && !ensure_row_blocks(ctx, p, "the rows' constraint states", r->row_state.count(), T, r->row_state, T)) return -1;
    if (!grow_tables(ctx, p, r->tokens, n_tokens)) return -1;
    if (lp && !ensure_logprob_blocks(ctx, p, T, r->tokens)) return -1;
    if (top && !ensure_top_blocks(ctx, p, T, r->tokens)) return -1;
    uint32_t w0[kSpecWords] = {0};
    w0[kSpecTok] = first_token, w0[kSpecPos] = start_pos, w0[kSpecWanted] = n_tokens, w0[kSpecMode] = model ? 2 : o.mode, w0[kSpecNgram] = ngram;
    w0[kSpecNDrafts] = std::min(n_drafts, r->max_seq), w0[kSpecStart] = start_pos, w0[kSpecHistLo] = o.n_history ? 0 : start_pos;
    w0[kSpecRunPos] = start_pos;
    // (the host arrays are the caller's or on this stack, and every copy below is waited for before the call returns)
    if (!CTX_CHECK(ctx, hipMemcpyAsync(r->spec, w0, sizeof(w0), hipMemcpyHostToDevice, s)) ||
        (o.n_history && !CTX_CHECK(ctx, hipMemcpyAsync(r->hist, o.history, (size_t)o.n_history * 4, hipMemcpyHostToDevice, s))) ||
        !CTX_CHECK(ctx, hipMemcpyAsync(r->hist + start_pos, &first_token, 4, hipMemcpyHostToDevice, s)) ||
        (w0[kSpecNDrafts] && !CTX_CHECK(ctx, hipMemcpyAsync(r->drafts, o.drafts, (size_t)w0[kSpecNDrafts] * 4, hipMemcpyHostToDevice, s))))
        return fail_after_copies(s);
    if (sampled && (!CTX_CHECK(ctx, hipMemcpyAsync(r->sparams, &sp, sizeof(sp), hipMemcpyHostToDevice, s)) || // (row 0: the one set every row reads)
                    !CTX_CHECK(ctx, hipMemsetAsync(r->tokens, 0xFF, (size_t)n_tokens * 8, s))))                // (-1: what a stop token leaves behind itself)
        return fail_after_copies(s);
    SpecArgs sa{r->spec, r->hist, r->drafts, r->tok_dev, r->tokens, r->bval, r->bidx, T, nblk, r->vocab, hist_cap, r->tokens_cap()};
    SampledTail tail; // (sampled form only; the greedy form launches none of it)
    if (sampled) { // rows of one sequence: row j samples at the step's run position + j and reads parameter row 0
        // (the constrained-rows select serves penalties on and off, as the constrained one does)
        tail = resident_tail(r, T, constrained ? kSelConstrainedRows : SampledTail::sel_of(false, penalized), SampledTail::kind_of(lp, top));
        tail.con = SampleConstraint{};
        if (constrained) { // one automaton — sequence 0's row of the table — and a state per row
            tail.con.rows = r->con_rows, tail.con.state = r->row_state;
            sa.con_row = r->con_rows, sa.con_state = r->con_state, sa.row_state = r->row_state;
        }
        sa.picks = r->picks, sa.sparams = r->sparams;
        tail.adv.picks = r->picks, tail.adv.pos_word = r->spec + kSpecRunPos, tail.adv.rows_per_seq = T; // (one sequence: all T rows are its)
        // (the `logprobs` field only) every row's value of its pick; the accept launch copies the emitted prefix
        tail.top.chosen.out = r->lp_rows, tail.top.chosen.picks = r->picks;
        // (the `top_logprobs` word only) every row's alternatives, likewise
        tail.top.top_tok = r->top_rows_tok, tail.top.top_val = r->top_rows_val, tail.top.shared_params = 1;
        // (penalised form only) a row's window is the call's history up to the run position and the candidates behind it
        tail.win.hist = r->hist, tail.win.cand = r->tok_dev, tail.win.lo_word = r->spec + kSpecHistLo;
    }
    if (lp) sa.lp_rows = r->lp_rows, sa.lp_out = r->lp;
    if (top) sa.top_rows_tok = r->top_rows_tok, sa.top_rows_val = r->top_rows_val, sa.top_tok_out = r->top_tok, sa.top_val_out = r->top_val;
    // the prep reads its position from the run words (the draft launch decides where the step runs) and its tokens from the candidates
    const Prep prep = prep_args(p, r->spec + kSpecRun, r->tok_dev);
    // (the model form) the draft's prep reads its own state words, as in zgml_hip_resident_decode: the draft launch and the
    // executions' advances write them; execution j's advance also writes candidate j + 1
    const Prep dprep = dr ? prep_args(draft, dr->state, dr->state /* the token is state[0] */) : Prep{};
    if (dr) sa.draft_state = dr->state;
    // the plan enters the step's graph through run_plan, as in resident_decode: many executions per call, with the dynamic words
    // written by the prep launch inside the graph (resident_prefill's enqueue replays the program's own graphs and would flush the
    // host mirror over them unless dyn_dirty is cleared per execution)
    auto one_step = [&](hipStream_t st) {
        launch_spec_draft(st, sa);
        for (uint32_t j = 0; dr && j < T; j++) {
            launch_resident_prep(st, dprep.a, dprep.total);
            run_plan(draft, st, 0, draft->plan.size());
            const DraftAdvance adv{dr->state, j + 1 < T ? r->tok_dev + j + 1 : nullptr};
            if (constrained) // the walk stands at row j's state; the advance writes row j + 1's and counts the draft
                launch_argmax_draft_constrained(st, dr->logits, dr->vocab, ctx->arg_val, ctx->arg_idx, adv, DraftConstraint{r->con_rows, r->row_state + j, T, r->spec + kSpecDrafted, kSpecWords});
            else
                launch_argmax_draft(st, dr->logits, dr->vocab, ctx->arg_val, ctx->arg_idx, adv);
        }
        launch_resident_prep(st, prep.a, prep.total);
        run_plan(p, st, 0, p->plan.size());
        if (sampled)
            tail.launch(st, r->logits, r->vocab);
        else
            launch_argmax_rows_stage1(st, r->logits, r->vocab, T, r->bval, r->bidx);
        launch_spec_accept(st, sa);
    };
    // (the model form) the pair's graphs serve this draft as it stands, and no other
    if (dr && (r->pair_draft != draft || r->pair_epoch != dr->graph_epoch)) {
        hipStreamSynchronize(s);
        free_pair_graphs(r);
        r->pair_draft = draft, r->pair_epoch = dr->graph_epoch;
    }
    const uint32_t pair_slot = sampled ? 1 + tail.form() : 0;
    GraphSlot& slot = dr ? r->pair_graph[pair_slot] : sampled ? r->sgraph[tail.form()] : r->graph;
    // (the sampled form waits, as the sampled loops: no copy from this stack frame in flight when the capture begins)
    capture_once(ctx, s, std::string(dr ? "resident_spec_model" : "resident_spec") + (sampled ? std::string("_") + kSampledFormNames[tail.form()] : std::string()), sampled, one_step, slot);
    // the host cannot know how many steps the drafts save: it launches the fewest that can finish, reads the count back, repeats
    // (`wanted` is read back with the words: a stop token of the sampled form sets it to the produced count, which ends the loop)
    uint32_t w1[kSpecWords] = {0};
    SampledCopyOut out{tail.kind};
    uint64_t steps_run = 0;
    bool ok = true;
    for (uint32_t produced = 0, wanted = n_tokens; ok && produced < wanted;) {
        const uint32_t round = (wanted - produced + T - 1) / T;
        replay(s, slot, round, one_step);
        steps_run += round;
        hipMemcpyAsync(w1, r->spec, sizeof(w1), hipMemcpyDeviceToHost, s);
        ok = CTX_CHECK(ctx, hipStreamSynchronize(s));
        // (every step with tokens left emits at least one — unless the constraint's state allows no token: the call is then
        // finished, wanted == produced)
        if (ok && w1[kSpecProduced] <= produced && w1[kSpecWanted] != w1[kSpecProduced]) {
            ctx->fail(who + ": a round of verify steps produced nothing");
            ok = false;
        }
        produced = w1[kSpecProduced], wanted = std::min(w1[kSpecWanted], n_tokens);
    }
    if (ok) {
        hipMemcpyAsync(tokens_out, r->tokens, (size_t)n_tokens * 8, hipMemcpyDeviceToHost, s);
        out.download(s, r, n_tokens);
        ok = CTX_CHECK(ctx, hipStreamSynchronize(s));
    }
    ok = ok && ctx->handoff_ok(who.c_str());
    const uint32_t made = ok ? std::min(w1[kSpecProduced], n_tokens) : 0;
    const auto produced = [&](uint64_t e) { return e < made ? (int64_t)e : -1; };
    out.keep(ctx, n_tokens, top_logprobs_count(sp.top_logprobs, r->vocab), produced, produced);
    if (ok && stats) *stats = zgml_spec_stats{w1[kSpecSteps], w1[kSpecDrafted], w1[kSpecAccepted], 0};
    if (ok && n_produced) *n_produced = made;
    // per step [draft] [prep] [plan] [argmax stage 1] [accept], or the sampled tail in the place of the argmax stage
    resident_end(p, steps_run, p->plan.size() + 3 + (sampled ? tail.launches() : 1));
    if (dr) resident_end(draft, steps_run * T, draft->plan.size() + 3); // per step T x { [prep] [plan] [argmax x 2] }
    return ok ? 0 : -1;
}

} // namespace

extern "C" {

int zgml_hip_resident_decode_speculative_model(zgml_hip_ctx* ctx, zgml_hip_program* target, zgml_hip_program* draft, uint32_t first_token, uint32_t start_pos,
                                               uint32_t n_tokens, const uint32_t* history, uint32_t n_history, const zgml_sampling* sampling, int64_t* tokens_out,
                                               uint32_t* n_produced, zgml_spec_stats* stats) {
    const zgml_spec_decode opt{history, n_history, 0, nullptr, 0, 0};
    return spec_decode(ctx, target, "resident_decode_speculative_model", first_token, start_pos, n_tokens, &opt, sampling != nullptr, sampling, tokens_out, n_produced,
                       stats, false, true, draft);
}

int zgml_hip_resident_decode_speculative_model_constrained(zgml_hip_ctx* ctx, zgml_hip_program* target, zgml_hip_program* draft, uint32_t first_token,
                                                           uint32_t start_pos, uint32_t n_tokens, const uint32_t* history, uint32_t n_history,
                                                           const zgml_sampling* sampling, int64_t* tokens_out, uint32_t* n_produced, zgml_spec_stats* stats) {
    if (!ctx) return -1;
    if (!sampling) { // (the verify step is the constrained one, which is a sampled one: top_k = 1 is its greedy form)
        if (n_produced) *n_produced = 0;
        ctx->fail("resident_decode_speculative_model_constrained: sampling is NULL (the constrained verify step is a sampled one: top_k = 1 is the greedy form)");
        return -1;
    }
    const zgml_spec_decode opt{history, n_history, 0, nullptr, 0, 0};
    return spec_decode(ctx, target, "resident_decode_speculative_model_constrained", first_token, start_pos, n_tokens, &opt, true, sampling, tokens_out, n_produced,
                       stats, true, true, draft);
}

int zgml_hip_resident_decode_speculative(zgml_hip_ctx* ctx, zgml_hip_program* p, uint32_t first_token, uint32_t start_pos, uint32_t n_tokens,
                                         const zgml_spec_decode* opt, int64_t* tokens_out, zgml_spec_stats* stats) {
    return spec_decode(ctx, p, "resident_decode_speculative", first_token, start_pos, n_tokens, opt, false, nullptr, tokens_out, nullptr, stats);
}

int zgml_hip_resident_decode_speculative_sampled(zgml_hip_ctx* ctx, zgml_hip_program* p, uint32_t first_token, uint32_t start_pos, uint32_t n_tokens,
                                                 const zgml_spec_decode* opt, const zgml_sampling* sampling, int64_t* tokens_out, uint32_t* n_produced,
                                                 zgml_spec_stats* stats) {
    return spec_decode(ctx, p, "resident_decode_speculative_sampled", first_token, start_pos, n_tokens, opt, true, sampling, tokens_out, n_produced, stats);
}

int zgml_hip_resident_decode_speculative_constrained(zgml_hip_ctx* ctx, zgml_hip_program* p, uint32_t first_token, uint32_t start_pos, uint32_t n_tokens,
                                                     const zgml_spec_decode* opt, const zgml_sampling* sampling, int64_t* tokens_out, uint32_t* n_produced,
                                                     zgml_spec_stats* stats) {
    return spec_decode(ctx, p, "resident_decode_speculative_constrained", first_token, start_pos, n_tokens, opt, true, sampling, tokens_out, n_produced, stats, true);
}

} // extern "C"

namespace {

// Speculative decode of n_seqs sequences over a batched plan with Ts = tokens_per_seq columns per sequence (contract:
// include/zgml_hip.h; rules: spec.h), both forms, as spec_decode() serves the single-sequence ones. Per step [draft, B sequences]
// [prep, B Ts columns] [plan] [argmax stage 1 over B Ts rows] [accept + advance, B sequences], one graph of its own; sequence b's
// device state is spec_decode()'s, at row b of every block. The sampled form (`sampled`:
// zgml_hip_resident_decode_batch_speculative_sampled) has [select] [merge + pick] over the B Ts rows in the place of the argmax
// stage — one launch more; logits row r is candidate row r % Ts of sequence r / Ts (kernels.h: SampleAdvance) and reads that
// sequence's parameter set —, graphs of its own in the slots no other sampled loop can use on such a plan, and a stop token ends
// its sequence early: the others go on. Everything the greedy form enqueues is what it enqueued before the sampled one existed.
// `honours_constraint` (zgml_hip_resident_decode_batch_speculative_constrained; spec.h: UNDER A CONSTRAINT): the sampled form, and
// with a constraint attached to any sequence the constrained one, as in spec_decode() — the same launches with the constrained-rows
// select in the place of the select (row b Ts + j: sequence b's automaton, its own state word), the draft and the accept launch
// of every attached sequence also walking its automaton, graphs of their own; the rows of a sequence without one are free
// (spec.h: kSpecRowFree). A reached state without a token finishes its sequence as a stop token does: the others go on. With
// nothing attached it is the sampled form to the launch.
// `model` (zgml_hip_resident_decode_batch_speculative_model; spec.h: DRAFTS FROM A MODEL): every sequence's candidates come from
// `draft`, a batched plan of the same context, vocabulary and n_seqs with ONE column per sequence, executed Ts times between the
// draft launch and the prep —
//   [begin, B] Ts x { [draft batch prep] [draft plan] [argmax stage 1, (nblk, B)] [stage 2 + draft advance, (1, B)] } [prep] [plan] ... [accept, B]
// one graph launch, a linear chain, Ts draft executions whatever B. The draft's device state is its batched loop's (token and
// position rows of bstate), its stage-1 pairs its own bval / bidx. Either form of the verify step; `per_seq` carries the
// histories alone. The graphs belong to the pair (Resident::pair_graph: spec_decode() cannot use them on a batched plan); each
// program's profile counts its own launches. A sequence that has its count hands the draft (hist[pos], pos) and the draft idles
// from there, Ts columns on: both programs need start_pos + n_tokens + Ts <= max_seq.
int spec_decode_batch(zgml_hip_ctx* ctx, zgml_hip_program* p, const std::string& who, const uint32_t* first_tokens, const uint32_t* start_pos,
                      const uint32_t* n_tokens, uint32_t max_tokens, const zgml_spec_decode* per_seq, bool sampled, const zgml_sampling* sampling,
                      int64_t* tokens_out, uint32_t* n_produced, zgml_spec_stats* stats, bool honours_constraint = false, bool model = false,
                      zgml_hip_program* draft = nullptr) {
    if (!ctx || !p) return -1;
    Resident* r = p->resident;
    if (!r || !r->n_seqs || !p->n_seqs) {
        ctx->fail(who + ": not a batched program with a resident set-up (zgml_hip_program_set_sequences, then zgml_hip_resident_setup)");
        return -1;
    }
    const uint32_t B = r->n_seqs, Ts = r->tokens_per_seq;
    if (Ts < 2) {
        ctx->fail(who + ": the batched plan holds one column per sequence (a verify step needs tokens_per_seq >= 2)");
        return -1;
    }
    if (!honours_constraint && refuse_constrained(ctx, p, who.c_str())) return -1;
    const bool constrained = honours_constraint && r->n_con != 0;
    Resident* const dr = model && draft ? draft->resident : nullptr;
    if (model) { // what the call asks of the two programs beside that
        const char* why = !p->shard_points.empty() ? "the target is a sharded program (gather points attached)"
                          : !draft ? "no draft program" : draft == p ? "the draft is the target program itself" : draft->ctx != p->ctx ? "the draft belongs to another context"
                          : !dr ? "the draft has no resident set-up (zgml_hip_resident_setup first)"
                          : !dr->n_seqs || !draft->n_seqs ? "the draft is a plain plan (a batched draft is needed: zgml_hip_program_set_sequences)"
                          : dr->tokens_per_seq != 1 ? "the draft must hold one column per sequence (tokens_per_seq = 1)"
                          : dr->n_seqs != B ? "the draft has another n_seqs than the target"
                          : !draft->shard_points.empty() ? "the draft is a sharded program (gather points attached)"
                          : dr->vocab != r->vocab ? "the draft has another vocabulary than the target" : nullptr;
        if (why) {
            ctx->fail(who + ": " + why);
            return -1;
        }
        if (has_constraint(draft)) { // (forced tokens would have to be placed between the draft executions: not served)
            ctx->fail(who + ": a constraint is attached to the draft program (detach it first)");
            return -1;
        }
    }
    if (!first_tokens || !start_pos || !n_tokens || (max_tokens && !tokens_out)) {
        ctx->fail(who + ": NULL array (first_tokens, start_pos, n_tokens, or tokens_out with max_tokens > 0)");
        return -1;
    }
    if (sampled && !sampling) {
        ctx->fail(who + ": no sampling parameters (one zgml_sampling per sequence)");
        return -1;
    }
    std::vector<SpecRequest> req(B);
    std::vector<SampleParamsDev> sp(sampled ? B : 0);
    uint32_t most = 0;
    bool penalized = false; // one sequence with penalties: the penalised select for all (a row without them computes what it did)
    bool lp = false;        // ... and one with log-probabilities: the two launches for all (a sequence that did not ask is not copied out)
    for (uint32_t b = 0; b < B; b++) {
        const std::string seq = who + " (sequence " + std::to_string(b) + ")";
        if (n_tokens[b] > max_tokens) {
            ctx->fail(seq + ": n_tokens exceeds max_tokens");
            return -1;
        }
        if (!spec_request(ctx, r, seq, first_tokens[b], start_pos[b], n_tokens[b], Ts, true, per_seq ? per_seq + b : nullptr, &req[b])) return -1;
        if (dr && (uint64_t)start_pos[b] + n_tokens[b] + Ts > dr->max_seq) { // (the target's bound: the draft stores the same Ts columns per step)
            ctx->fail(seq + ": start_pos + n_tokens + tokens_per_seq exceeds the draft's max_seq");
            return -1;
        }
        if (sampled) {
            if (!sampling_params(ctx, seq, sampling + b, r->vocab, r->vocab, &sp[b], RecentOf::Spec)) return -1;
            penalized = penalized || sp[b].pen_active, lp = lp || sampling[b].logprobs;
        }
        most = std::max(most, n_tokens[b]);
    }
    for (uint64_t i = 0; i < (uint64_t)B * max_tokens; i++) tokens_out[i] = -1;
    for (uint32_t b = 0; stats && b < B; b++) stats[b] = zgml_spec_stats{0, 0, 0, 0};
    for (uint32_t b = 0; n_produced && b < B; b++) n_produced[b] = 0;
    if (!most) return 0;
    hipSetDevice(ctx->device);
    hipStream_t s = ctx->stream;
    // every sequence's first start and its last possible one: the position it idles at
    resident_begin(p, [&] {
        return positions_in_bounds(p, Ts, [&](uint32_t i) { return start_pos[p->op_seq[i]]; }) &&
               positions_in_bounds(p, Ts, [&](uint32_t i) { return start_pos[p->op_seq[i]] + n_tokens[p->op_seq[i]]; });
    });
    // ... and the first and the last possible position of a draft execution: the Ts-th of a step that idles at the end position
    if (dr) resident_begin(draft, [&] {
        return positions_in_bounds(draft, 1, [&](uint32_t i) { return start_pos[draft->op_seq[i]]; }) &&
               positions_in_bounds(draft, 1, [&](uint32_t i) { return start_pos[draft->op_seq[i]] + n_tokens[draft->op_seq[i]] + Ts - 1; });
    });
    const uint32_t nblk = (uint32_t)argmax_batch_blocks(r->vocab), hist_cap = r->max_seq + 1, n_words = B * kSpecWords + 1, rows = B * Ts;
    if (!ensure_row_blocks(ctx, p, "the batched verify step's blocks", r->bhist.count() / hist_cap * Ts, rows, r->bspec, n_words, r->bhist, (size_t)B * hist_cap,
                           r->bdrafts, (size_t)B * r->max_seq))
        return -1;
    // (sampled form only) every block for B Ts logits rows: the select keys, a parameter row per sequence (the block has one per
    // logits row), the rows' picks, the rows' values and the block pairs; the emitted values lie as the tokens do
    if (sampled && (!ensure_sample_blocks(ctx, p, rows) || !ensure_row_blocks(ctx, p, "the rows' picks", r->picks.count(), rows, r->picks, rows))) return -1;
    if (constrained && !ensure_row_blocks(ctx, p, "the rows' constraint states", r->row_state.count(), rows, r->row_state, rows)) return -1;
    if (!grow_tables(ctx, p, r->btokens, (size_t)B * max_tokens)) return -1;
    if (lp && !ensure_logprob_blocks(ctx, p, rows, r->btokens)) return -1;
    std::vector<uint32_t> w0(n_words, 0), w1(n_words, 0);
    w0[(size_t)B * kSpecWords] = max_tokens; // row length of the device token table of this call
    bool up = true;
    for (uint32_t b = 0; up && b < B; b++) {
        uint32_t* w = w0.data() + (size_t)b * kSpecWords;
        const zgml_spec_decode& o = req[b].o;
        w[kSpecTok] = first_tokens[b], w[kSpecPos] = start_pos[b], w[kSpecWanted] = n_tokens[b], w[kSpecMode] = model ? 2 : o.mode, w[kSpecNgram] = req[b].ngram;
        w[kSpecNDrafts] = std::min(req[b].n_drafts, r->max_seq), w[kSpecStart] = start_pos[b], w[kSpecHistLo] = o.n_history ? 0 : start_pos[b];
        w[kSpecRunPos] = start_pos[b];
        uint32_t* const hist = r->bhist + (size_t)b * hist_cap;
        // (the host arrays are the caller's or this call's, and every copy below is waited for before the call returns)
        up = (!o.n_history || CTX_CHECK(ctx, hipMemcpyAsync(hist, o.history, (size_t)o.n_history * 4, hipMemcpyHostToDevice, s))) &&
             CTX_CHECK(ctx, hipMemcpyAsync(hist + start_pos[b], first_tokens + b, 4, hipMemcpyHostToDevice, s)) &&
             (!w[kSpecNDrafts] || CTX_CHECK(ctx, hipMemcpyAsync(r->bdrafts + (size_t)b * r->max_seq, o.drafts, (size_t)w[kSpecNDrafts] * 4, hipMemcpyHostToDevice, s)));
    }
    if (!up || !CTX_CHECK(ctx, hipMemcpyAsync(r->bspec, w0.data(), w0.size() * 4, hipMemcpyHostToDevice, s)) ||
        !CTX_CHECK(ctx, hipMemsetAsync(r->btokens, 0xFF, (size_t)B * max_tokens * 8, s)) || // (-1: what a sequence leaves behind its count, or its stop token)
        (sampled && !CTX_CHECK(ctx, hipMemcpyAsync(r->sparams, sp.data(), sp.size() * sizeof(SampleParamsDev), hipMemcpyHostToDevice, s)))) {
        return fail_after_copies(s); // (w0 and sp are read by copies that may be in flight)
    }
    SpecBatchArgs sa{{r->bspec, r->bhist, r->bdrafts, r->tok_dev, r->btokens, r->bval, r->bidx, Ts, nblk, r->vocab, hist_cap, 0 /* the device word */}, B, r->max_seq};
    SampledTail tail; // (sampled form only; the greedy form launches none of it)
    if (sampled) { // row b Ts + j: sequence b's parameter row, its run position + j, its history and candidates
        // (the constrained-rows select serves penalties on and off, as in spec_decode())
        tail = resident_tail(r, rows, constrained ? kSelConstrainedRows : SampledTail::sel_of(false, penalized), SampledTail::kind_of(lp, false)); // (the alternatives are not kept: include/zgml_hip.h)
        tail.con = SampleConstraint{};
        if (constrained) { // sequence b's automaton — its row of the table — for its Ts rows, and a state per row
            tail.con.rows = r->con_rows, tail.con.state = r->row_state;
            sa.a.con_row = r->con_rows, sa.a.con_state = r->con_state, sa.a.row_state = r->row_state;
        }
        sa.a.picks = r->picks, sa.a.sparams = r->sparams;
        tail.adv.picks = r->picks, tail.adv.pos_word = r->bspec + kSpecRunPos, tail.adv.rows_per_seq = Ts, tail.adv.pos_stride = kSpecWords;
        // (the `logprobs` field only) every row's value of its pick; the accept launch copies each sequence's emitted prefix
        tail.top.chosen.out = r->lp_rows, tail.top.chosen.picks = r->picks;
        // (penalised form only) a row's window is its sequence's history up to the run position and the candidates behind it
        tail.win.hist = r->bhist, tail.win.hist_stride = hist_cap, tail.win.cand = r->tok_dev, tail.win.lo_word = r->bspec + kSpecHistLo;
        if (lp) sa.a.lp_rows = r->lp_rows, sa.a.lp_out = r->lp;
    }
    const ResidentBatchSpecPrepArgs prep{r->embed, r->cos, r->sin, r->tok_in, r->mask, r->rope_bufs, r->dyn_kind, r->dyn_base, r->dyn_stride, r->dyn_seq,
                                         p->dyn_dev, r->bspec, r->tok_dev, r->d, r->max_seq, r->dh, r->n_rope, (uint32_t)p->ops.size(), B, Ts};
    // (the model form) the draft's prep reads the token and position rows of its own batched state, as in
    // zgml_hip_resident_decode_batch: the draft launch and the executions' advances write them; execution j's advance also writes
    // candidate j + 1 of every sequence. The stage-1 pairs of its B rows go to the draft's own scratch
    const BatchPrep dprep = dr ? batch_prep_args(draft) : BatchPrep{};
    if (dr) sa.a.draft_state = dr->bstate, sa.a.draft_pos = B;
    auto one_step = [&](hipStream_t st) {
        launch_spec_batch_draft(st, sa);
        for (uint32_t j = 0; dr && j < Ts; j++) {
            launch_resident_batch_prep(st, dprep.a, dprep.total);
            run_plan(draft, st, 0, draft->plan.size());
            launch_argmax_batch_draft(st, dr->logits, dr->vocab, dr->bval, dr->bidx, DraftAdvance{dr->bstate, j + 1 < Ts ? r->tok_dev + j + 1 : nullptr, B, Ts});
        }
        launch_resident_batch_spec_prep(st, prep, r->prep_total);
        run_plan(p, st, 0, p->plan.size());
        if (sampled)
            tail.launch(st, r->logits, r->vocab);
        else
            launch_argmax_rows_stage1(st, r->logits, r->vocab, rows, r->bval, r->bidx);
        launch_spec_batch_accept(st, sa);
    };
    // (the model form) the pair's graphs serve this draft as it stands, and no other
    if (dr && (r->pair_draft != draft || r->pair_epoch != dr->graph_epoch)) {
        hipStreamSynchronize(s);
        free_pair_graphs(r);
        r->pair_draft = draft, r->pair_epoch = dr->graph_epoch;
    }
    GraphSlot& slot = dr ? r->pair_graph[sampled ? 1 + tail.form() : 0] : sampled ? r->sgraph[tail.form()] : r->bspec_graph;
    // (as the batched loops: no pageable copy in flight when the capture begins)
    capture_once(ctx, s, std::string(dr ? "resident_batch_spec_model" : "resident_batch_spec") + (sampled ? std::string("_") + kSampledFormNames[tail.form()] : std::string()), true,
                 one_step, slot);
    // the host cannot know how many steps the drafts save: it launches the fewest that can finish the sequence with the most
    // tokens left, reads the counts back, repeats. (`wanted` is read back with the words: a stop token of the sampled form sets
    // its sequence's to the produced count, which shortens the round)
    std::vector<uint32_t> produced(B, 0), wanted(n_tokens, n_tokens + B);
    uint64_t steps_run = 0;
    bool ok = true;
    while (ok) {
        uint32_t round = 0;
        for (uint32_t b = 0; b < B; b++) round = std::max(round, (wanted[b] - produced[b] + Ts - 1) / Ts);
        if (!round) break;
        replay(s, slot, round, one_step);
        steps_run += round;
        hipMemcpyAsync(w1.data(), r->bspec, w1.size() * 4, hipMemcpyDeviceToHost, s);
        ok = CTX_CHECK(ctx, hipStreamSynchronize(s));
        for (uint32_t b = 0; ok && b < B; b++) {
            const uint32_t now = std::min(w1[(size_t)b * kSpecWords + kSpecProduced], n_tokens[b]);
            const uint32_t left = std::max(now, std::min(w1[(size_t)b * kSpecWords + kSpecWanted], n_tokens[b])); // (the device's word: a stop token or a dead end has cut it)
            // (every step of a sequence with tokens left emits at least one — unless its constraint's state allows no token: the
            // sequence is then finished, wanted == produced on the device, and it idles from here on)
            if (produced[b] < wanted[b] && now <= produced[b] && left != now) {
                ctx->fail(who + ": a round of verify steps produced nothing (sequence " + std::to_string(b) + ")");
                ok = false;
            }
            produced[b] = now, wanted[b] = left;
        }
    }
    SampledCopyOut out{tail.kind};
    if (ok) {
        hipMemcpyAsync(tokens_out, r->btokens, (size_t)B * max_tokens * 8, hipMemcpyDeviceToHost, s); // (the device rows are max_tokens long too)
        out.download(s, r, (uint64_t)B * max_tokens);
        ok = CTX_CHECK(ctx, hipStreamSynchronize(s));
    }
    ok = ok && ctx->handoff_ok(who.c_str());
    // [n_seqs][max_tokens] values, as tokens_out: a sequence that did not ask, and every entry behind a count, keeps the NaN
    out.keep(ctx, (uint64_t)B * max_tokens, 0, [&](uint64_t e) {
        const uint32_t b = (uint32_t)(e / max_tokens), i = (uint32_t)(e % max_tokens);
        return ok && sampling[b].logprobs && i < produced[b] ? (int64_t)e : -1; }, [](uint64_t) { return (int64_t)-1; });
    for (uint32_t b = 0; ok && b < B; b++) {
        const uint32_t* w = w1.data() + (size_t)b * kSpecWords;
        if (stats) stats[b] = zgml_spec_stats{w[kSpecSteps], w[kSpecDrafted], w[kSpecAccepted], 0};
        if (n_produced) n_produced[b] = produced[b];
    }
    // per step [draft] [prep] [plan] [argmax stage 1] [accept], or the sampled tail in the place of the argmax stage
    resident_end(p, steps_run, p->plan.size() + 3 + (sampled ? tail.launches() : 1));
    if (dr) resident_end(draft, steps_run * Ts, draft->plan.size() + 3); // per step Ts x { [batched prep] [plan] [argmax x 2] }
    return ok ? 0 : -1;
}

} // namespace

extern "C" {

int zgml_hip_resident_decode_batch_speculative_model(zgml_hip_ctx* ctx, zgml_hip_program* target, zgml_hip_program* draft, const uint32_t* first_tokens,
                                                     const uint32_t* start_pos, const uint32_t* n_tokens, uint32_t max_tokens, const uint32_t* const* histories,
                                                     const uint32_t* n_history, const zgml_sampling* sampling, int64_t* tokens_out, uint32_t* n_produced,
                                                     zgml_spec_stats* stats) {
    // the histories as the requests of the batched siblings carry them (mode and drafts are not the caller's here)
    std::vector<zgml_spec_decode> opt(target && target->resident ? target->resident->n_seqs : 0);
    for (size_t b = 0; b < opt.size(); b++) opt[b] = zgml_spec_decode{histories ? histories[b] : nullptr, n_history ? n_history[b] : 0, 0, nullptr, 0, 0};
    return spec_decode_batch(ctx, target, "resident_decode_batch_speculative_model", first_tokens, start_pos, n_tokens, max_tokens, opt.empty() ? nullptr : opt.data(),
                             sampling != nullptr, sampling, tokens_out, n_produced, stats, false, true, draft);
}

int zgml_hip_resident_decode_batch_speculative(zgml_hip_ctx* ctx, zgml_hip_program* p, const uint32_t* first_tokens, const uint32_t* start_pos,
                                               const uint32_t* n_tokens, uint32_t max_tokens, const zgml_spec_decode* per_seq, int64_t* tokens_out,
                                               zgml_spec_stats* stats) {
    return spec_decode_batch(ctx, p, "resident_decode_batch_speculative", first_tokens, start_pos, n_tokens, max_tokens, per_seq, false, nullptr, tokens_out, nullptr, stats);
}

int zgml_hip_resident_decode_batch_speculative_sampled(zgml_hip_ctx* ctx, zgml_hip_program* p, const uint32_t* first_tokens, const uint32_t* start_pos,
                                                       const uint32_t* n_tokens, uint32_t max_tokens, const zgml_spec_decode* per_seq,
                                                       const zgml_sampling* sampling, int64_t* tokens_out, uint32_t* n_produced, zgml_spec_stats* stats) {
    return spec_decode_batch(ctx, p, "resident_decode_batch_speculative_sampled", first_tokens, start_pos, n_tokens, max_tokens, per_seq, true, sampling, tokens_out,
                             n_produced, stats);
}

int zgml_hip_resident_decode_batch_speculative_constrained(zgml_hip_ctx* ctx, zgml_hip_program* p, const uint32_t* first_tokens, const uint32_t* start_pos,
                                                           const uint32_t* n_tokens, uint32_t max_tokens, const zgml_spec_decode* per_seq,
                                                           const zgml_sampling* sampling, int64_t* tokens_out, uint32_t* n_produced, zgml_spec_stats* stats) {
    return spec_decode_batch(ctx, p, "resident_decode_batch_speculative_constrained", first_tokens, start_pos, n_tokens, max_tokens, per_seq, true, sampling,
                             tokens_out, n_produced, stats, true);
}

} // extern "C"
