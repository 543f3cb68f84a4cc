// tsvpp_table.cpp -- persistent frame tables (include/tsvpp.h): the pointer triples of many frames kept on the device, set once and converted from in runs.
#include "tsvpp_host.h"

using namespace tsvpp;

struct tsvpp_table {
    tsvpp_ctx *ctx = nullptr;   // null once the context has been destroyed (tsvpp_destroy releases the table's device memory; tsvpp_table_destroy then only frees the host side)
    int capacity = 0;
    uint64_t *dev = nullptr;    // three columns of `capacity` entries: y | uv | out
    std::vector<tsvpp_nv12> in; // host mirror (geometry checks, alignment decisions, the two-pass formats): updated only after an upload has been enqueued in full
    std::vector<void *> outs;
    std::vector<uint8_t> set;   // entry has been set
    bool have_geom = false;
    tsvpp_nv12 geom = {};
    std::mutex mu;
    // Upload staging: until round 5 every upload was copied out of ONE pinned mirror that the next tsvpp_table_set rewrote at once -- a second set of the
    // same entries before the first upload had run made the first copy pick up the second call's pointers, against the stream ordering the header promises.  Each upload now
    // has its own pinned slot, reused only after the event recorded behind its copies has completed; a slot that is too small is replaced (the old one freed: its event is done).
    struct Slot {
        uint64_t *buf = nullptr;
        size_t entries = 0; // capacity in table entries (3 columns each)
        hipEvent_t done = nullptr;
        bool busy = false;
    };
    static constexpr int kSlots = 4;
    Slot slots[kSlots];
    int next_slot = 0;
};

static void table_release_device(tsvpp_table *t) { // caller has selected the device
    if (t->dev) (void)hipFree(t->dev);
    t->dev = nullptr;
    for (auto &sl : t->slots) {
        if (sl.done) (void)hipEventDestroy(sl.done);
        if (sl.buf) (void)hipHostFree(sl.buf);
        sl = tsvpp_table::Slot();
    }
}

// Frame tables the caller has not destroyed when its context goes: their device memory goes with the context, their handles stay valid for tsvpp_table_destroy.
void tsvpp::ctx_release_tables(tsvpp_ctx *ctx) { // caller has selected the device
    std::lock_guard<std::mutex> lk(ctx->tables_mu);
    for (tsvpp_table *t : ctx->tables) {
        std::lock_guard<std::mutex> tl(t->mu);
        table_release_device(t);
        t->ctx = nullptr;
    }
    ctx->tables.clear();
}

extern "C" {

int tsvpp_table_create(tsvpp_ctx *ctx, int capacity, tsvpp_table **out_table) {
    if (!ctx || !out_table || capacity < 1 || capacity > (1 << 24)) return TSVPP_ERROR;
    *out_table = nullptr;
    DeviceGuard guard(ctx);
    if (guard.status != TSVPP_OK) return guard.status;
    tsvpp_table *t = new tsvpp_table;
    t->ctx = ctx;
    t->capacity = capacity;
    const size_t bytes = (size_t)3 * capacity * sizeof(uint64_t);
    hipError_t e = hipMalloc((void **)&t->dev, bytes);
    if (e == hipSuccess) e = hipMemset(t->dev, 0, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (t->dev) (void)hipFree(t->dev);
        delete t;
        return (int)e;
    }
    t->in.resize((size_t)capacity);
    t->outs.assign((size_t)capacity, nullptr);
    t->set.assign((size_t)capacity, 0);
    {
        std::lock_guard<std::mutex> lk(ctx->tables_mu);
        ctx->tables.insert(t);
    }
    *out_table = t;
    return TSVPP_OK;
}

void tsvpp_table_destroy(tsvpp_table *table) {
    if (!table) return;
    if (tsvpp_ctx *ctx = table->ctx) { // (a table that outlived its context was already released by tsvpp_destroy)
        {
            std::lock_guard<std::mutex> lk(ctx->tables_mu);
            ctx->tables.erase(table);
        }
        DeviceGuard guard(ctx);
        table_release_device(table);
    }
    delete table;
}

int tsvpp_table_set(tsvpp_table *table, int first, int n, const tsvpp_nv12 *in, void *const *outs, void *stream) {
    if (!table || !table->ctx || !in || !outs || first < 0 || n < 0 || (long)first + n > table->capacity) return TSVPP_ERROR;
    if (n == 0) return TSVPP_OK;
    std::lock_guard<std::mutex> lk(table->mu);
    const tsvpp_nv12 g = table->have_geom ? table->geom : in[0];
    bool a4, v16; // (not a table's business: a conversion classes its run of entries)
    // one geometry per table, as one per batch (tsvpp_convert_batch)
    const int sts = check_frames(n, in, outs, g.width, g.height, pitch_or_width(g.pitch_y, g.width), pitch_or_width(g.pitch_uv, g.width), 0, 0, a4, v16);
    if (sts != TSVPP_OK) return sts;
    DeviceGuard guard(table->ctx);
    if (guard.status != TSVPP_OK) return guard.status;
    // Not on a capturing stream (include/tsvpp.h): the copies would become graph nodes that read a staging slot at every replay, long after later uploads have
    // rewritten it, and the event behind them a captured event that nobody can wait for -- the slot would stay busy for good.  Refused before a slot is touched.
    // (the NULL stream is never queried: asking the legacy stream while another stream captures in global mode invalidates that capture)
    if (stream) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing((hipStream_t)stream, &cs) != hipSuccess) (void)hipGetLastError();
        else if (cs != hipStreamCaptureStatusNone) return TSVPP_UNSUPPORTED;
    }
    // this upload's staging slot: wait for the copies that last read it, grow it if needed
    tsvpp_table::Slot &sl = table->slots[table->next_slot];
    if (sl.busy) {
        const hipError_t e = hipEventSynchronize(sl.done);
        if (e != hipSuccess) {
            // the wait itself was refused: the event is of no use any more.  The slot is reset -- a fresh event on its next use, its buffer kept -- and this call
            // reports the error; the next upload takes the slot as free instead of failing for as long as the table lives.
            (void)hipGetLastError();
            (void)hipEventDestroy(sl.done);
            sl.done = nullptr;
            sl.busy = false;
            table->next_slot = (table->next_slot + 1) % tsvpp_table::kSlots; // (its buffer rests for three uploads: a copy may still be reading it)
            return (int)e;
        }
        sl.busy = false;
    }
    if (sl.entries < (size_t)n) {
        if (sl.buf) (void)hipHostFree(sl.buf);
        sl.buf = nullptr;
        sl.entries = 0;
        size_t want = 64;
        while (want < (size_t)n) want *= 2;
        const hipError_t e = hipHostMalloc((void **)&sl.buf, 3 * want * sizeof(uint64_t), hipHostMallocDefault);
        if (e != hipSuccess) { (void)hipGetLastError(); return (int)e; }
        sl.entries = want;
    }
    if (!sl.done) {
        const hipError_t e = hipEventCreateWithFlags(&sl.done, hipEventDisableTiming);
        if (e != hipSuccess) { (void)hipGetLastError(); return (int)e; } // (reported here: the thread's next launch must not find it)
    }
    for (int f = 0; f < n; f++) {
        sl.buf[f] = (uint64_t)(uintptr_t)in[f].y;
        sl.buf[(size_t)n + f] = (uint64_t)(uintptr_t)in[f].uv;
        sl.buf[2 * (size_t)n + f] = (uint64_t)(uintptr_t)outs[f];
    }
    const size_t cap = (size_t)table->capacity;
    for (int col = 0; col < 3; col++) { // the three column ranges: asynchronous, ordered on `stream`
        const hipError_t e = hipMemcpyAsync(table->dev + col * cap + first, sl.buf + (size_t)col * n, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice, (hipStream_t)stream);
        if (e != hipSuccess) {
            // a column may already be on its way: the entries are in an unknown state on the device -> they count as never set (tsvpp_convert_table refuses them)
            for (int f = 0; f < n; f++) table->set[(size_t)first + f] = 0;
            (void)hipEventRecord(sl.done, (hipStream_t)stream);
            sl.busy = true;
            return (int)e;
        }
    }
    const hipError_t er = hipEventRecord(sl.done, (hipStream_t)stream);
    if (er != hipSuccess) { // cannot tell when the slot is free again: wait for the stream now
        (void)hipStreamSynchronize((hipStream_t)stream);
    } else {
        sl.busy = true;
    }
    table->next_slot = (table->next_slot + 1) % tsvpp_table::kSlots;
    for (int f = 0; f < n; f++) { // the host mirror follows the device: only now
        const size_t k = (size_t)first + f;
        table->in[k] = in[f];
        table->outs[k] = outs[f];
        table->set[k] = 1;
    }
    table->geom = g;
    table->have_geom = true;
    return TSVPP_OK;
}

int tsvpp_convert_table(tsvpp_ctx *ctx, const tsvpp_table *table, int first, int n, const tsvpp_params *p, void *stream) {
    if (!ctx || !table || table->ctx != ctx || !p || first < 0 || n < 0 || (long)first + n > table->capacity) return TSVPP_ERROR;
    if (n == 0) return TSVPP_OK;
    for (int f = 0; f < n; f++)
        if (!table->set[(size_t)first + f]) return TSVPP_ERROR; // an entry that was never set
    const size_t cap = (size_t)table->capacity;
    TableCols cols;
    cols.y = table->dev + first;
    cols.uv = table->dev + cap + first;
    cols.out = table->dev + 2 * cap + first;
    return convert_impl(ctx, n, table->in.data() + first, p, table->outs.data() + first, stream, cols);
}

} // extern "C"
