// Chain diagnostics (include/lmc_abi.h "Chain diagnostics"; device/chaindiag.hip): rows of chosen chains gathered on the device, traces of them over the
// lock steps of a render, and the table of chain-steps per (launch kind, technique).  Host code around three launch functions: the state hangs off
// lmc_ctx::diag, and context.cpp calls the hooks below from its step path, each behind `if (c->diag)`.
#include <cstring>

#include "context.h"

namespace lmc_host {

constexpr size_t kTableWords = 3 * 13 * 13 * 2;

struct ChainDiag {
    DevBuf<unsigned char> kindOf;  // per rank-local chain: the launch of the chain's current step (k_latch_kind), zero until a step has run
    // trace
    bool open = false;
    int n = 0, capacity = 0, nSteps = 0;
    long long firstStep = 0, dropped = 0;
    DevBuf<int> ids;     // rank-local ids of the tracked chains
    DevBuf<float> rows;  // capacity x n x LMC_ROW_WORDS
    // step table
    bool tableOn = false;
    DevBuf<unsigned long long> table;  // [3][13][13][2]
};

namespace {

ChainDiag *Get(lmc_ctx *c) {
    if (!c->diag) c->diag = new ChainDiag;
    return c->diag;
}
template <class T>
void AllocNamed(DevBuf<T> &b, size_t count, const char *who, const char *what) {
    try {
        b.Alloc(count);
    } catch (const std::exception &) {
        (void)hipGetLastError();
        b.p = nullptr, b.n = 0;
        throw std::runtime_error(std::string(who) + ": cannot allocate " + std::to_string((unsigned long long)(count * sizeof(T))) + " bytes of device memory for " + what);
    }
}
// the latch has one byte per chain of the population in force
void SizeLatch(lmc_ctx *c, ChainDiag *d, const char *who) {
    if (d->kindOf.n != (size_t)c->N) AllocNamed(d->kindOf, (size_t)c->N, who, "the step-kind latch");
}
// GLOBAL chain ids -> rank-local ones; throws on an id outside [chainBegin, chainBegin + N)
std::vector<int> LocalIds(const lmc_ctx *c, const int *ids, int n, const char *who) {
    if (n <= 0) throw std::runtime_error(std::string(who) + ": n > 0 chain ids expected");
    if (!ids) throw std::runtime_error(std::string(who) + ": chain_ids is NULL");
    std::vector<int> local((size_t)n);
    for (int k = 0; k < n; k++) {
        if (ids[k] < c->chainBegin || ids[k] >= c->chainBegin + c->N)
            throw std::runtime_error(std::string(who) + ": chain id " + std::to_string(ids[k]) + " is outside this context's chains [" + std::to_string(c->chainBegin) + ", " +
                                     std::to_string(c->chainBegin + c->N) + ")");
        local[(size_t)k] = ids[k] - c->chainBegin;
    }
    return local;
}
void CloseTrace(ChainDiag *d) {
    d->open = false;
    d->n = d->capacity = d->nSteps = 0;
    d->firstStep = d->dropped = 0;
    d->ids.Free(), d->rows.Free();
}

}  // namespace

void DiagStepBegin(lmc_ctx *c, int cur) {
    ChainDiag *d = c->diag;
    if (!d->open && !d->tableOn) return;
    SizeLatch(c, d, "chain diagnostics");
    LaunchLatchKind(c->A, c->lists[cur][0].p, c->lists[cur][1].p, c->lists[cur][2].p, c->listCounts[cur].p, d->kindOf.p, c->stream);
}

void DiagStepEnd(lmc_ctx *c) {
    ChainDiag *d = c->diag;
    if (!d->open && !d->tableOn) return;
    if (d->kindOf.n != (size_t)c->N) return;  // switched on between the two halves of a step: counts from the next one
    if (d->tableOn) LaunchStepTable(c->A, d->kindOf.p, d->table.p, c->stream);
    if (d->open) {
        if (d->nSteps >= d->capacity) d->dropped++;
        else {
            if (d->nSteps == 0) d->firstStep = c->stepsSinceInit + 1;  // StepPhase2 counts the step behind this hook
            LaunchChainRows(c->A, 0, d->ids.p, d->n, d->kindOf.p, d->rows.p + (size_t)d->nSteps * d->n * LMC_ROW_WORDS, c->stream);
            d->nSteps++;
        }
    }
}

bool DiagNeedsLockStep(const lmc_ctx *c) { return c->diag->open || c->diag->tableOn; }
bool DiagStepTableOn(const lmc_ctx *c) { return c->diag->tableOn; }

void DiagChainsReset(lmc_ctx *c) {
    ChainDiag *d = c->diag;
    HIP_CHECK(hipStreamSynchronize(c->stream));
    CloseTrace(d);
    d->kindOf.Free();
}

void DiagSetStepTable(lmc_ctx *c, bool on) {
    if (!on && !c->diag) return;
    ChainDiag *d = Get(c);
    if (on && !d->table.p) {
        HIP_CHECK(hipSetDevice(c->device));
        AllocNamed(d->table, kTableWords, "step_table", "the step table");
    }
    if (on && !d->tableOn && !d->open && d->kindOf.p) {  // the latch may be stale: nothing kept it up while both diagnostics were off
        HIP_CHECK(hipSetDevice(c->device));
        HIP_CHECK(hipMemsetAsync(d->kindOf.p, 0, d->kindOf.n, c->stream));
    }
    d->tableOn = on;
}

void DiagFree(lmc_ctx *c) {
    if (c->diag) {
        (void)hipSetDevice(c->device);
        if (c->stream) (void)hipStreamSynchronize(c->stream);
    }
    delete c->diag;
    c->diag = nullptr;
}

}  // namespace lmc_host

extern "C" {

int lmc_chain_rows(lmc_ctx *c, int which, const int *chain_ids, int n, float *out) {
    LMC_TRY
    if (c->N <= 0) throw std::runtime_error("lmc_chain_rows: the context holds no chains (lmc_chains_init or lmc_checkpoint_load first)");
    if (which != 0 && which != 1) throw std::runtime_error("lmc_chain_rows: which is 0 (current states) or 1 (init states)");
    if (!out) throw std::runtime_error("lmc_chain_rows: out is NULL");
    const std::vector<int> local = LocalIds(c, chain_ids, n, "lmc_chain_rows");
    HIP_CHECK(hipSetDevice(c->device));
    DevBuf<int> ids;
    DevBuf<float> rows;
    AllocNamed(ids, (size_t)n, "lmc_chain_rows", "the chain ids");
    AllocNamed(rows, (size_t)n * LMC_ROW_WORDS, "lmc_chain_rows", "the rows");
    HIP_CHECK(hipMemcpyAsync(ids.p, local.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
    const ChainDiag *d = c->diag;
    const unsigned char *kindOf = d && d->open && d->kindOf.n == (size_t)c->N ? d->kindOf.p : nullptr;
    LaunchChainRows(c->A, which, ids.p, n, kindOf, rows.p, c->stream);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(out, rows.p, (size_t)n * LMC_ROW_WORDS * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    return 0;
    LMC_CATCH(-1)
}

// the pending splat lists (A.curSplat) of chosen chains, gathered on the device: what row word 15 only counts
int lmc_chain_splats(lmc_ctx *c, const int *chain_ids, int n, int cap, float *out, int *counts) {
    LMC_TRY
    if (c->N <= 0) throw std::runtime_error("lmc_chain_splats: the context holds no chains (lmc_chains_init or lmc_checkpoint_load first)");
    static_assert(LMC_SPLAT_MAX_ENTRIES == MAXCONTRIB, "include/lmc_abi.h names the length a pending list can have");
    if (cap < 1 || cap > MAXCONTRIB) throw std::runtime_error("lmc_chain_splats: cap is 1 .. " + std::to_string(MAXCONTRIB) + " entries per chain");
    if (!out || !counts) throw std::runtime_error("lmc_chain_splats: out or counts is NULL");
    const std::vector<int> local = LocalIds(c, chain_ids, n, "lmc_chain_splats");
    HIP_CHECK(hipSetDevice(c->device));
    DevBuf<int> ids, cnt;
    DevBuf<float> rows;
    AllocNamed(ids, (size_t)n, "lmc_chain_splats", "the chain ids");
    AllocNamed(cnt, (size_t)n, "lmc_chain_splats", "the list lengths");
    AllocNamed(rows, (size_t)n * cap * LMC_SPLAT_WORDS, "lmc_chain_splats", "the entries");
    HIP_CHECK(hipMemcpyAsync(ids.p, local.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
    LaunchChainSplats(c->A, c->filmLayers ? c->splatLabels.p : nullptr, ids.p, n, cap, rows.p, cnt.p, c->stream);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(out, rows.p, (size_t)n * cap * LMC_SPLAT_WORDS * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipMemcpyAsync(counts, cnt.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    return 0;
    LMC_CATCH(-1)
}

int lmc_chain_trace_begin(lmc_ctx *c, const int *chain_ids, int n, int capacity_steps) {
    LMC_TRY
    if (c->N <= 0) throw std::runtime_error("lmc_chain_trace_begin: the context holds no chains (lmc_chains_init or lmc_checkpoint_load first)");
    if (c->diag && c->diag->open) throw std::runtime_error("lmc_chain_trace_begin: a trace is open already (lmc_chain_trace_end first)");
    if (capacity_steps <= 0) throw std::runtime_error("lmc_chain_trace_begin: capacity_steps > 0 expected");
    const std::vector<int> local = LocalIds(c, chain_ids, n, "lmc_chain_trace_begin");
    HIP_CHECK(hipSetDevice(c->device));
    ChainDiag *d = Get(c);
    DevBuf<int> ids;
    DevBuf<float> rows;
    AllocNamed(ids, (size_t)n, "lmc_chain_trace_begin", "the chain ids");
    {  // not zero-filled: a row is written before it is counted
        const size_t count = (size_t)capacity_steps * (size_t)n * LMC_ROW_WORDS;
        if (hipMalloc((void **)&rows.p, count * sizeof(float)) != hipSuccess) {
            (void)hipGetLastError();
            rows.p = nullptr;
            throw std::runtime_error("lmc_chain_trace_begin: cannot allocate " + std::to_string((unsigned long long)(count * sizeof(float))) + " bytes of device memory for the trace buffer");
        }
        rows.n = count;
    }
    SizeLatch(c, d, "lmc_chain_trace_begin");
    HIP_CHECK(hipMemcpy(ids.p, local.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice));
    if (!d->tableOn) HIP_CHECK(hipMemsetAsync(d->kindOf.p, 0, d->kindOf.n, c->stream));  // no step of this trace has run: kind 0 (with the table on the latch is current)
    std::swap(d->ids.p, ids.p), std::swap(d->ids.n, ids.n);
    std::swap(d->rows.p, rows.p), std::swap(d->rows.n, rows.n);
    d->n = n, d->capacity = capacity_steps, d->nSteps = 0, d->firstStep = 0, d->dropped = 0;
    d->open = true;
    return 0;
    LMC_CATCH(-1)
}

int lmc_chain_trace_read(lmc_ctx *c, float *rows, int cap_steps, long long *first_step, int *n_steps, long long *dropped) {
    LMC_TRY
    ChainDiag *d = c->diag;
    if (!d || !d->open) throw std::runtime_error("lmc_chain_trace_read: no trace is open (lmc_chain_trace_begin first)");
    if (rows && cap_steps < d->nSteps)
        throw std::runtime_error("lmc_chain_trace_read: the trace holds " + std::to_string(d->nSteps) + " steps, rows has room for " + std::to_string(cap_steps));
    if (first_step) *first_step = d->nSteps ? d->firstStep : c->stepsSinceInit + 1;
    if (n_steps) *n_steps = d->nSteps;
    if (dropped) *dropped = d->dropped;
    if (!rows) return 0;
    HIP_CHECK(hipSetDevice(c->device));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    if (d->nSteps) HIP_CHECK(hipMemcpy(rows, d->rows.p, (size_t)d->nSteps * d->n * LMC_ROW_WORDS * sizeof(float), hipMemcpyDeviceToHost));
    d->nSteps = 0, d->firstStep = 0, d->dropped = 0;
    return 0;
    LMC_CATCH(-1)
}

int lmc_chain_trace_end(lmc_ctx *c) {
    LMC_TRY
    ChainDiag *d = c->diag;
    if (!d || !d->open) throw std::runtime_error("lmc_chain_trace_end: no trace is open");
    HIP_CHECK(hipSetDevice(c->device));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    CloseTrace(d);
    return 0;
    LMC_CATCH(-1)
}

int lmc_step_table(lmc_ctx *c, long long *out, int clear) {
    LMC_TRY
    if (!out) throw std::runtime_error("lmc_step_table: out is NULL");
    ChainDiag *d = c->diag;
    if (!d || !d->table.p) {  // never switched on: an empty table
        memset(out, 0, kTableWords * sizeof(long long));
        return 0;
    }
    HIP_CHECK(hipSetDevice(c->device));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    HIP_CHECK(hipMemcpy(out, d->table.p, kTableWords * sizeof(long long), hipMemcpyDeviceToHost));
    if (clear) HIP_CHECK(hipMemsetAsync(d->table.p, 0, kTableWords * sizeof(long long), c->stream));
    return 0;
    LMC_CATCH(-1)
}

}  // extern "C"
