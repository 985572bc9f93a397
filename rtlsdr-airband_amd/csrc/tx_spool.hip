/* csrc/tx_spool.hip -- transmission spool (airband_hip_set_transmission_spool / _collect_transmissions / _spool_flush, and the mixer spool's
 * airband_hip_set_mixer_spool / _collect_mixer_transmissions / _mixer_spool_flush over the mixer gate's rows: "channel" below is then a mixer, "the gate" the
 * mixer gate, "the encoder" the mixer pack, and a row is W * wave_batch samples): the encoded rows of every open transmission kept in a row pool on the GPU, the reference's closing rule for `split_on_transmission` file sinks applied once per batch, and finished
 * transmissions handed over as 48-byte records and one contiguous run of rows.  The definition is include/airband_hip.h's ("transmission spool");
 * capi.transmission_spool_reference() is the same in plain Python.  Integers only: records and audio are checked as bytes.
 *
 * What is held where.  Per channel a SpoolChan (the running record and the head and tail of the transmission's chain of pool rows); next[pool row] links a chain;
 * free_stack[0 .. free_top) are the rows nobody holds; fin[] is a ring of max_records finished records (reserved[0] carries the chain's head while a record
 * waits); one SpoolCtl holds the counts.  Which pool row a transmission gets is not observable; WHO gets one when the pool runs dry is, so rows are handed
 * out by rank in ascending channel order -- rank r takes free_stack[F - 1 - r] -- and ranks come from ballots and per-workgroup counts as in gate.hip, never
 * from an atomic cursor.  Rows that come BACK (a dropped transmission, a collect) are pushed through an atomic cursor: the order of the pushes only decides
 * which row holds which audio.
 *
 * Four launches per batch on a handle with a spool, behind the encoder on the same stream (driver_gate.cpp, launch_gate_behind_mix, called by run_back_half); none on a handle without one:
 *   spool_scan_kernel    one lane per channel: phase A's verdict and "spooled and selected by the gate", one ballot each per wavefront, one count each per
 *                        workgroup; thread 0 fixes what the step sees of the finished list (room, where records go) and clears the step's sum;
 *   spool_close_kernel   the same lanes: a closing channel's rank among the closers -> its record into the ring while rank < room, else dropped and its
 *                        chain pushed back; the last workgroup's first thread books the step's totals;
 *   spool_append_kernel  the same lanes: rank among the gate's channels (is the row among the first max_rows?) and among the spooled ones (is there a pool
 *                        row?), the transmission opened and advanced, the row's place written to the copy list;
 *   spool_copy_kernel    the copy list's rows from the encoder's buffer into the pool, a workgroup per row, and the free count lowered.
 * A value that one of these kernels reads from the control block is never written by the same kernel, so no workgroup can see a half-advanced step.
 * Flush is scan + close with every open transmission closing.  Collect is three launches: spool_export_kernel (ONE workgroup: prefix sums of n_rows over the
 * waiting records, the longest prefix that fits export_rows, the records with their row offsets), spool_walk_kernel (one lane per exported transmission walks
 * its chain into the source-row list and pushes the rows back) and spool_gather_kernel (row i of the export buffer = pool row src[i]).
 *
 * Rows are dense and wave_batch is only a multiple of four, so a row of 1 000 G.711 bytes starts on a multiple of 8, not 16: lanes move 8 bytes where the row's
 * bytes are a multiple of 8 (1 000, 2 000, 4 000 are, and so is every mixer row: W * wave_batch * bytes is 1 000 .. 8 000), else 4.  The encoder's row is read once: non-temporal load; the store is ordinary.
 *
 * Every count and index read from device memory is clamped to its buffer before anything is indexed with it: the free count, the list's head and count, chain
 * links, n_rows, the step's stored count, the copy list's entries.
 */
#include <hip/hip_runtime.h>

#include "common.h"
#include "kernels.h"

namespace airband {

namespace {
constexpr int SPOOL_BLOCK = 1024; /* channels (lanes) per workgroup of the per-channel passes: gate.hip's GATE_BLOCK, whose masks and counts the append pass reads */
constexpr int SPOOL_WAVES = SPOOL_BLOCK / 64;
typedef unsigned sp_v2u __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int sp_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

/* the channel's rank among the set bits of a fleet-wide mask: the counts of the workgroups in front, the wavefronts in front, the lanes in front
 * (gate_index_kernel's scheme); called by every thread of a workgroup.  SET: a kernel that asks for two ranks gives each its own LDS.  *total: the workgroup's
 * base + its own count, which in the last workgroup is the fleet's */
template <int SET>
__device__ __forceinline__ int sp_rank(unsigned long long m, const int* block_count, int* total) {
    __shared__ int wave_count[SPOOL_WAVES];
    __shared__ int base;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    int before = 0;
    for (int j = threadIdx.x; j < (int)blockIdx.x; j += SPOOL_BLOCK) before += block_count[j];
    if (before) atomicAdd(&base, before);
    if (lane == 0) wave_count[w] = __popcll(m);
    __syncthreads();
    int pos = base, n = base;
    for (int i = 0; i < SPOOL_WAVES; i++) {
        pos += i < w ? wave_count[i] : 0;
        n += wave_count[i];
    }
    *total = n;
    return pos + __popcll(m & ((1ull << lane) - 1ull));
}

/* one ballot per wavefront and one count per workgroup (gate_select_kernel's second half) */
__device__ __forceinline__ void sp_publish(bool bit, int c, int n_ch, unsigned long long* mask, int* block_count, int* wave_count) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long m = __ballot(bit);
    if (lane == 0) {
        if (c < n_ch) mask[c >> 6] = m;
        wave_count[w] = __popcll(m);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0;
        for (int i = 0; i < SPOOL_WAVES; i++) n += wave_count[i];
        block_count[blockIdx.x] = n;
    }
    __syncthreads();
}

/* a chain of n rows from `head` pushed back on the free stack, and (src != null) listed at src[0 .. n) */
__device__ __forceinline__ void sp_release_chain(const SpoolArgs& a, int head, int n, int* src) {
    if (n <= 0) return;
    const int at = atomicAdd(&a.ctl->free_top, n);
    int row = head;
    for (int u = 0; u < n; u++) {
        row = sp_clamp(row, 0, a.pool_rows - 1);
        if (src) src[u] = row;
        if (at + u >= 0 && at + u < a.pool_rows) a.free_stack[at + u] = row;
        row = a.next[row];
    }
}
}  // namespace

template <bool FLUSH>
__device__ __forceinline__ void spool_scan(const SpoolArgs& a) {
    __shared__ int wave_count[SPOOL_WAVES];
    const int c = blockIdx.x * SPOOL_BLOCK + threadIdx.x, lane = threadIdx.x & 63;
    bool closes = false, appends = false;
    if (c < a.n_ch && a.spool[c]) {
        const SpoolChan& st = a.chan[c];
        if (st.open) {
            const uint32_t age = a.k - st.open_batch, quiet = a.k - st.last_batch;
            closes = FLUSH || (age > a.min_batches && quiet > a.idle_batches) || age > a.max_batches;
        }
        appends = !FLUSH && ((a.gate_mask[c >> 6] >> lane) & 1ull);
    }
    sp_publish(closes, c, a.n_ch, a.close_mask, a.close_count, wave_count);
    if (!FLUSH) sp_publish(appends, c, a.n_ch, a.app_mask, a.app_count, wave_count);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        SpoolCtl& t = *a.ctl;
        const int count = sp_clamp(t.fin_count, 0, a.max_records), head = sp_clamp(t.fin_head, 0, a.max_records - 1);
        t.fin_count = count;
        t.fin_head = head;
        t.room = a.max_records - count;
        t.fin_tail = (int)(((long)head + count) % a.max_records);
        t.n_stored_step = 0;
        t.free_top = sp_clamp(t.free_top, 0, a.pool_rows);
    }
}

__global__ __launch_bounds__(SPOOL_BLOCK) void spool_scan_kernel(SpoolArgs a) { spool_scan<false>(a); }
__global__ __launch_bounds__(SPOOL_BLOCK) void spool_flush_scan_kernel(SpoolArgs a) { spool_scan<true>(a); }

/* reason: 0 = by the rule (IDLE or MAX), else AIRBAND_SPOOL_FLUSH */
__global__ __launch_bounds__(SPOOL_BLOCK) void spool_close_kernel(SpoolArgs a, int reason) {
    const int c = blockIdx.x * SPOOL_BLOCK + threadIdx.x, lane = threadIdx.x & 63;
    const unsigned long long m = (c - lane) < a.n_ch ? a.close_mask[c >> 6] : 0ull;
    int total = 0;
    const int rank = sp_rank<0>(m, a.close_count, &total);
    const int room = a.ctl->room, tail = a.ctl->fin_tail;
    if (c < a.n_ch && ((m >> lane) & 1ull)) {
        SpoolChan& st = a.chan[c];
        const int n = (int)(st.n_rows < a.max_batches + 1u ? st.n_rows : a.max_batches + 1u);
        if (rank < room) {
            airband_hip_transmission r;
            r.channel = c;
            r.open_batch = st.open_batch;
            r.last_batch = st.last_batch;
            r.close_batch = a.k;
            r.n_rows = (uint32_t)n;
            r.n_lost = st.n_lost;
            r.n_clipped = st.n_clipped;
            r.peak = st.peak;
            r.first = st.first;
            r.end = st.end;
            const bool idle = a.k - st.open_batch > a.min_batches && a.k - st.last_batch > a.idle_batches;
            r.reason = (uint16_t)(reason ? reason : (idle ? AIRBAND_SPOOL_IDLE : AIRBAND_SPOOL_MAX));
            r.row_offset = 0;
            r.reserved[0] = (uint32_t)st.head;
            r.reserved[1] = st.flags;
            a.fin[(int)(((long)tail + rank) % a.max_records)] = r;
        } else {
            sp_release_chain(a, st.head, n, nullptr); /* dropped: the list is full */
        }
        st.open = 0;
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        SpoolCtl& t = *a.ctl;
        const int kept = total < room ? total : room;
        t.fin_count += kept;
        t.finished_total += (unsigned long long)kept;
        t.dropped += (unsigned long long)(total - kept);
        t.open_now -= (unsigned long long)total;
    }
}

__global__ __launch_bounds__(SPOOL_BLOCK) void spool_append_kernel(SpoolArgs a) {
    const int c = blockIdx.x * SPOOL_BLOCK + threadIdx.x, lane = threadIdx.x & 63;
    const bool wave_in = (c - lane) < a.n_ch;
    const unsigned long long mg = wave_in ? a.gate_mask[c >> 6] : 0ull, ms = wave_in ? a.app_mask[c >> 6] : 0ull;
    int n_selected = 0, n_spooled = 0;
    const int pos = sp_rank<0>(mg, a.gate_count, &n_selected); /* the row's place in the gate's list, had the list no end */
    const int j = sp_rank<1>(ms, a.app_count, &n_spooled);     /* its rank among the spooled rows: the storable ones are a prefix of them */
    (void)n_selected;
    (void)n_spooled;
    const int F = sp_clamp(a.ctl->free_top, 0, a.pool_rows);
    const bool mine = c < a.n_ch && ((ms >> lane) & 1ull);
    bool opened = false, stored = false;
    if (mine) {
        SpoolChan st = a.chan[c];
        if (!st.open) {
            st.open_batch = a.k;
            st.n_rows = st.n_lost = st.n_clipped = 0;
            st.flags = 0;
            st.peak = 0;
            st.first = (uint16_t)a.wave_batch;
            st.end = 0;
            st.open = 1;
            st.head = st.tail = -1;
            opened = true;
        }
        stored = pos < a.max_rows && j < F;
        if (stored) {
            const int row = sp_clamp(a.free_stack[F - 1 - j], 0, a.pool_rows - 1);
            a.next[row] = -1;
            if (st.n_rows == 0 || st.tail < 0)
                st.head = row;
            else
                a.next[sp_clamp(st.tail, 0, a.pool_rows - 1)] = row;
            st.tail = row;
            const airband_hip_audio_row info = a.enc_info[pos];
            st.peak = info.peak > st.peak ? info.peak : st.peak;
            const uint32_t sum = st.n_clipped + info.n_clipped;
            st.n_clipped = sum < st.n_clipped ? 0xFFFFFFFFu : sum;
            if (st.n_rows == 0) st.first = info.first;
            st.end = info.end;
            st.flags |= info.reserved; /* a mixer's stereo flag at this step; a channel's record carries 0 */
            st.n_rows++;
            a.copy_list[2 * j] = pos;
            a.copy_list[2 * j + 1] = row;
        } else {
            st.n_lost++;
        }
        st.last_batch = a.k;
        a.chan[c] = st;
    }
    /* the step's sums: integer additions, whose order does not show.  Nothing in this kernel reads them */
    const unsigned long long mo = __ballot(opened), mst = __ballot(stored), ml = __ballot(mine && !stored);
    if (lane == 0) {
        if (mo) atomicAdd(&a.ctl->open_now, (unsigned long long)__popcll(mo));
        if (mst) atomicAdd(&a.ctl->n_stored_step, (int)__popcll(mst));
        if (ml) atomicAdd(&a.ctl->rows_lost, (unsigned long long)__popcll(ml));
    }
}

/* row r of the copy list: the encoder's row -> its pool row.  A workgroup takes rows blockIdx.x, blockIdx.x + gridDim.x, ...: how many there are is on the device */
template <class V>
__device__ __forceinline__ void spool_copy_rows(const SpoolArgs& a) {
    const int cap = a.max_rows < a.pool_rows ? a.max_rows : a.pool_rows;
    const int n = sp_clamp(a.ctl->n_stored_step, 0, cap), nvec = a.row_bytes / (int)sizeof(V);
    for (int r = blockIdx.x; r < n; r += gridDim.x) {
        const int from = sp_clamp(a.copy_list[2 * r], 0, a.max_rows - 1), to = sp_clamp(a.copy_list[2 * r + 1], 0, a.pool_rows - 1);
        const V* src = reinterpret_cast<const V*>(a.enc_audio + (long)from * a.row_bytes);
        V* dst = reinterpret_cast<V*>(a.pool + (long)to * a.row_bytes);
        for (int v = threadIdx.x; v < nvec; v += 256) dst[v] = __builtin_nontemporal_load(src + v);
    }
}

/* ... and the rows the step took leave the free stack: the one count the copy's workgroups read (n_stored_step) is not touched here */
__global__ __launch_bounds__(256) void spool_copy_kernel(SpoolArgs a) {
    if (a.row_bytes % 8 == 0)
        spool_copy_rows<sp_v2u>(a);
    else
        spool_copy_rows<unsigned>(a);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        SpoolCtl& t = *a.ctl;
        const int cap = a.max_rows < a.pool_rows ? a.max_rows : a.pool_rows;
        const int n = sp_clamp(t.n_stored_step, 0, cap < t.free_top ? cap : t.free_top);
        t.free_top -= n;
        t.rows_stored += (unsigned long long)n;
    }
}

/* ONE workgroup walks the waiting records in chunks of 1 024 with a carried total (band_pack.h's scheme): record i is exported iff the rows up to and including
 * it fit export_rows -- n_rows is not negative, so those are a prefix of the list */
__global__ __launch_bounds__(SPOOL_BLOCK) void spool_export_kernel(SpoolArgs a) {
    __shared__ int wave_total[2][SPOOL_WAVES];
    __shared__ int s_n, s_rows;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int count = sp_clamp(a.ctl->fin_count, 0, a.max_records), head = sp_clamp(a.ctl->fin_head, 0, a.max_records - 1);
    const int most = (int)(a.max_batches + 1u);
    if (tid == 0) s_n = s_rows = 0;
    __syncthreads(); /* also: every thread has read the list's head and count before thread 0 moves them */
    long carry = 0;
    int chunk = 0;
#pragma unroll 1
    for (int i0 = 0; i0 < count; i0 += SPOOL_BLOCK, chunk++) {
        const int i = i0 + tid;
        const int at = (int)(((long)head + i) % a.max_records);
        int n = i < count ? sp_clamp((int)a.fin[at].n_rows, 0, most) : 0;
        int incl = n;
#pragma unroll
        for (int dl = 1; dl < 64; dl <<= 1) {
            const int o = (int)__shfl_up((unsigned)incl, (unsigned)dl);
            if (lane >= dl) incl += o;
        }
        int* const tot = wave_total[chunk & 1];
        if (lane == 63) tot[wave] = incl;
        __syncthreads();
        long before = carry, all = 0;
        for (int w = 0; w < SPOOL_WAVES; w++) {
            const int v = tot[w];
            before += w < wave ? v : 0;
            all += v;
        }
        const long upto = before + incl;
        const bool fits = i < count && upto <= (long)a.export_rows;
        if (fits) {
            airband_hip_transmission r = a.fin[at];
            a.exp_head[i] = (int)r.reserved[0];
            r.n_rows = (uint32_t)n;
            r.row_offset = (uint32_t)(upto - n);
            r.reserved[0] = 0; /* the chain's head is the spool's own; reserved[1] is the record's: the OR of the stored rows' flags */
            a.exp_records[i] = r;
        }
        const unsigned long long mf = __ballot(fits); /* a prefix of the wavefront's lanes */
        if (mf && lane == __popcll(mf) - 1) {
            atomicMax(&s_n, i + 1);
            atomicMax(&s_rows, (int)upto);
        }
        carry += all;
    }
    __syncthreads();
    if (tid == 0) {
        SpoolCtl& t = *a.ctl;
        t.exp[0] = s_n;
        t.exp[1] = s_rows;
        t.exp[2] = count - s_n;
        t.fin_head = (int)(((long)head + s_n) % a.max_records);
        t.fin_count = count - s_n;
    }
}

/* one lane per exported transmission: its chain into the source-row list, its rows back on the free stack */
__global__ __launch_bounds__(256) void spool_walk_kernel(SpoolArgs a) {
    const int n = sp_clamp(a.ctl->exp[0], 0, a.max_records);
    for (int t = blockIdx.x * 256 + threadIdx.x; t < n; t += gridDim.x * 256) {
        const airband_hip_transmission r = a.exp_records[t];
        const int off = sp_clamp((int)r.row_offset, 0, a.export_rows);
        int rows = sp_clamp((int)r.n_rows, 0, (int)(a.max_batches + 1u));
        rows = rows < a.export_rows - off ? rows : a.export_rows - off;
        sp_release_chain(a, a.exp_head[t], rows, a.exp_src + off);
    }
}

template <class V>
__device__ __forceinline__ void spool_gather_rows(const SpoolArgs& a) {
    const int n = sp_clamp(a.ctl->exp[1], 0, a.export_rows), nvec = a.row_bytes / (int)sizeof(V);
    for (int r = blockIdx.x; r < n; r += gridDim.x) {
        const int from = sp_clamp(a.exp_src[r], 0, a.pool_rows - 1);
        const V* src = reinterpret_cast<const V*>(a.pool + (long)from * a.row_bytes);
        V* dst = reinterpret_cast<V*>(a.exp_audio + (long)r * a.row_bytes);
        for (int v = threadIdx.x; v < nvec; v += 256) __builtin_nontemporal_store(__builtin_nontemporal_load(src + v), dst + v);
    }
}

/* row i of the export buffer = pool row src[i]; read once here and read next by a copy engine: non-temporal both ways, as in gate_gather_kernel */
__global__ __launch_bounds__(256) void spool_gather_kernel(SpoolArgs a) {
    if (a.row_bytes % 8 == 0)
        spool_gather_rows<sp_v2u>(a);
    else
        spool_gather_rows<unsigned>(a);
}

namespace {
int spool_blocks(int n_ch) { return (n_ch + SPOOL_BLOCK - 1) / SPOOL_BLOCK; }
int spool_row_grid(int rows) { return rows < 1 ? 1 : (rows < 2048 ? rows : 2048); } /* eight workgroups of four wavefronts fill a CU; 256 CUs */
}  // namespace

void launch_spool_step(const SpoolArgs& a, hipStream_t stream) {
    const int nb = spool_blocks(a.n_ch);
    hipLaunchKernelGGL(spool_scan_kernel, dim3(nb), dim3(SPOOL_BLOCK), 0, stream, a);
    hipLaunchKernelGGL(spool_close_kernel, dim3(nb), dim3(SPOOL_BLOCK), 0, stream, a, 0);
    hipLaunchKernelGGL(spool_append_kernel, dim3(nb), dim3(SPOOL_BLOCK), 0, stream, a);
    hipLaunchKernelGGL(spool_copy_kernel, dim3(spool_row_grid(a.max_rows < a.pool_rows ? a.max_rows : a.pool_rows)), dim3(256), 0, stream, a);
}

void launch_spool_flush(const SpoolArgs& a, hipStream_t stream) {
    const int nb = spool_blocks(a.n_ch);
    hipLaunchKernelGGL(spool_flush_scan_kernel, dim3(nb), dim3(SPOOL_BLOCK), 0, stream, a);
    hipLaunchKernelGGL(spool_close_kernel, dim3(nb), dim3(SPOOL_BLOCK), 0, stream, a, (int)AIRBAND_SPOOL_FLUSH);
}

void launch_spool_collect(const SpoolArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(spool_export_kernel, dim3(1), dim3(SPOOL_BLOCK), 0, stream, a);
    const int nt = (a.max_records + 255) / 256;
    hipLaunchKernelGGL(spool_walk_kernel, dim3(nt < 1024 ? nt : 1024), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(spool_gather_kernel, dim3(spool_row_grid(a.export_rows)), dim3(256), 0, stream, a);
}

}  // namespace airband
