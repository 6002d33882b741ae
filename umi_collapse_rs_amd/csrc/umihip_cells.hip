// Cell calling over the triplets of a count matrix (umi_call_cells, the program's --cell-filter), gfx950: the
// columns (cells) whose molecule total reaches a threshold read off the sorted totals, their per-column table, the
// summary numbers and the filtered triplets.  No counterpart in the reference; the rules are STARsolo's
// --soloCellFilter CellRanger2.2 and TopCells, tests/cells_model.py (call_model) defines them.  Exact integer work
// on HBM streams, 64-lane waves, no MFMA.
//
// Input: nnz triplets (row, col, molecules, reads) sorted by col, then row, as umi_count_matrix leaves them.
//
//   sums       a lane per triplet, 1,024 per block.  It compares its (col, row) with its predecessor's -- not
//              strictly greater counts into the control block -- and its ids with n_rows / n_cols.  A segmented
//              inclusive scan by col over (molecules, reads, molecules > 0) inside the wave (six __shfl_up steps),
//              then the waves of a block hand the sum of the run that leaves them to the waves behind through LDS:
//              a run's last lane in the block holds what the block adds to it.  A run that begins and ends inside
//              the block is stored; one that crosses a block's edge is added with atomicAdd (u64, u64, u32) onto
//              the zeroed per-column arrays -- one atomic triple per block and run, integer sums, so the result is
//              the same in every run.  No thread walks a run: one column may hold every triplet.
//   keys       a lane per column: the total becomes a sort key (all n_cols of them, zeros included: indexing the
//              sorted totals from the top needs no compaction); the candidates (total >= 1), all molecules and all
//              reads are block-reduced into the control block.
//   sort       radix_sort_pairs_u64 over the bits a total can use, 32 + bits(nnz) (umihip_radix.hip).
//   threshold  one wave reads S[i] = sorted[n_cols - 1 - i] and writes t and m into the control block; the kernels
//              behind read t there -- no host round trip.
//   call       a lane per column: called = total >= 1 && total >= t; a flag for scan_inclusive_u64 (new_col), the key
//              called ? genes : 0 of a second sort (radix_sort_pairs_u32 over bits(n_rows) bits), block-reduced
//              sums of the called molecules and reads.
//   number     a lane per column: new_col from the scan.  One thread reads the two lower medians: the called
//              columns are exactly the top `called` elements of either sorted array (a called column has a gene).
//   compact    a lane per triplet: called[col] && molecules > 0 as a flag, scan_inclusive_u64, and a scatter of the
//              triplet with new_col[col] to its slot (nnz_out = the last value of the scan).
//
// One synchronisation, at the end, brings the control block and nnz_out.  Workspace per column: keys 2 x 8 (the
// buffer the sort leaves free holds the flags), values 2 x 4 (both sorts), the flags' scan 8, gene keys 2 x 4: 40
// bytes; per triplet: flag 8 and its scan 8: 16 bytes; and the sort's and the scan's tables.
#include <hip/hip_runtime.h>
#include <algorithm>

#include "umihip_internal.h"

namespace umihip {

namespace {

#define CELLS_TRY(expr)                          \
    do {                                         \
        const hipError_t e__ = (expr);           \
        if (e__ != hipSuccess) return -(int)e__; \
    } while (0)

constexpr int CELLS_SUM_THREADS = 1024, CELLS_SUM_WAVES = CELLS_SUM_THREADS / 64;
constexpr int CELLS_THREADS = 256, CELLS_WAVES = CELLS_THREADS / 64;

// the control block's words
enum { CC_BAD_ID = 0, CC_BAD_ORDER, CC_CANDIDATES, CC_ALL_MOL, CC_ALL_READS, CC_T, CC_M, CC_MOL, CC_READS, CC_CALLED,
       CC_MED_MOL, CC_MED_GENES, CC_WORDS };
static_assert(CC_WORDS == CELLS_CTL_WORDS, "the words the host reads");

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

struct CellsWs {
    unsigned long long *ctl;
    uint64_t *ka, *kb;   // the totals and their sort; the free one holds the columns' flags
    uint32_t *va, *vb;   // the values of both sorts
    uint64_t *incl;      // [n_cols] scan of the columns' flags
    uint32_t *ga, *gb;   // the gene keys and their sort
    uint64_t *tflag, *tincl; // [nnz] the triplets' flags and their scan
    void *radix_tmp, *scan_tmp;
    size_t radix_bytes, scan_bytes, total;
};
CellsWs cells_carve(void *ws, uint32_t nnz, uint32_t n_cols)
{
    CellsWs w;
    char *p = (char *)ws;
    size_t o = 0;
    auto take = [&](size_t bytes) {
        char *at = p + o;
        o += align256(bytes);
        return at;
    };
    w.ctl = (unsigned long long *)take(256);
    w.ka = (uint64_t *)take((size_t)n_cols * 8);
    w.kb = (uint64_t *)take((size_t)n_cols * 8);
    w.va = (uint32_t *)take((size_t)n_cols * 4);
    w.vb = (uint32_t *)take((size_t)n_cols * 4);
    w.incl = (uint64_t *)take((size_t)n_cols * 8);
    w.ga = (uint32_t *)take((size_t)n_cols * 4);
    w.gb = (uint32_t *)take((size_t)n_cols * 4);
    w.tflag = (uint64_t *)take((size_t)nnz * 8);
    w.tincl = (uint64_t *)take((size_t)nnz * 8);
    w.radix_bytes = radix_sort_temp_bytes(n_cols);
    w.radix_tmp = take(w.radix_bytes);
    w.scan_bytes = std::max(scan_temp_bytes(n_cols), scan_temp_bytes(nnz));
    w.scan_tmp = take(w.scan_bytes);
    w.total = o;
    return w;
}

__global__ __launch_bounds__(CELLS_SUM_THREADS) void cells_sum_kernel(const uint32_t *__restrict__ row, const uint32_t *__restrict__ col,
                                                                      const uint32_t *__restrict__ molecules,
                                                                      const uint64_t *__restrict__ reads, uint32_t nnz, uint32_t n_rows,
                                                                      uint32_t n_cols, unsigned long long *cell_molecules,
                                                                      unsigned long long *cell_reads, uint32_t *cell_genes,
                                                                      unsigned long long *ctl)
{
    __shared__ unsigned long long tail_mol[CELLS_SUM_WAVES], tail_reads[CELLS_SUM_WAVES];
    __shared__ uint32_t tail_genes[CELLS_SUM_WAVES], has_head[CELLS_SUM_WAVES];
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    const int lane = (int)(tid & 63u);
    const uint64_t i = (uint64_t)blockIdx.x * CELLS_SUM_THREADS + tid;
    const bool valid = i < nnz;
    uint32_t r = 0, c = 0xFFFFFFFFu, g = 0;
    unsigned long long mol = 0, rd = 0;
    if (valid) {
        r = row[i];
        c = col[i];
        mol = molecules[i];
        rd = reads[i];
        g = mol != 0;
    }
    uint32_t pc = __shfl_up(c, 1), pr = __shfl_up(r, 1), nc = __shfl_down(c, 1);
    if (lane == 0 && valid && i > 0) {
        pc = col[i - 1];
        pr = row[i - 1];
    }
    if (lane == 63) nc = i + 1 < nnz ? col[i + 1] : 0xFFFFFFFFu;
    if (valid && (r >= n_rows || c >= n_cols)) atomicAdd(ctl + CC_BAD_ID, 1ull);
    if (valid && i > 0 && !(pc < c || (pc == c && pr < r))) atomicAdd(ctl + CC_BAD_ORDER, 1ull);
    const bool head = valid && (i == 0 || pc != c);
    const bool last = valid && (i + 1 >= nnz || nc != c); // the run ends here
    for (int d = 1; d < 64; d <<= 1) { // inclusive scan inside runs of one column
        const unsigned long long um = __shfl_up(mol, d), ur = __shfl_up(rd, d);
        const uint32_t ug = __shfl_up(g, d), uc = __shfl_up(c, d);
        if (lane >= d && uc == c) {
            mol += um;
            rd += ur;
            g += ug;
        }
    }
    const unsigned long long heads = __ballot(head);
    const unsigned long long upto = lane == 63 ? ~0ull : (2ull << lane) - 1ull;
    const bool in_first = (heads & upto) == 0ull; // the run this lane is in came in from the wave before
    if (lane == 63) { // what leaves the wave (worth nothing where the run ends here: the next wave starts with a head)
        tail_mol[wave] = mol;
        tail_reads[wave] = rd;
        tail_genes[wave] = g;
        has_head[wave] = heads != 0ull;
    }
    __syncthreads();
    bool from_outside = in_first; // ... and from the block before
    if (in_first) {
        for (int w = (int)wave - 1; w >= 0; w--) {
            mol += tail_mol[w];
            rd += tail_reads[w];
            g += tail_genes[w];
            if (has_head[w]) {
                from_outside = false;
                break;
            }
        }
    }
    // a run's last lane in this block holds what the block adds to it
    if (valid && c < n_cols && (last || tid == CELLS_SUM_THREADS - 1)) {
        if (last && !from_outside) {
            cell_molecules[c] = mol;
            cell_reads[c] = rd;
            cell_genes[c] = g;
        } else {
            atomicAdd(cell_molecules + c, mol);
            atomicAdd(cell_reads + c, rd);
            atomicAdd(cell_genes + c, g);
        }
    }
}

// the sum of three words over a block of CELLS_THREADS, good in thread 0
__device__ __forceinline__ void block_sum3(unsigned long long &a, unsigned long long &b, unsigned long long &c)
{
    __shared__ unsigned long long part[3][CELLS_WAVES];
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_down(a, o);
        b += __shfl_down(b, o);
        c += __shfl_down(c, o);
    }
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) {
        part[0][wave] = a;
        part[1][wave] = b;
        part[2][wave] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = b = c = 0;
        for (int w = 0; w < CELLS_WAVES; w++) {
            a += part[0][w];
            b += part[1][w];
            c += part[2][w];
        }
    }
}

__global__ __launch_bounds__(CELLS_THREADS) void cells_keys_kernel(const uint64_t *__restrict__ cell_molecules,
                                                                   const uint64_t *__restrict__ cell_reads, uint32_t n_cols,
                                                                   uint64_t *__restrict__ key, uint32_t *__restrict__ val,
                                                                   unsigned long long *ctl)
{
    unsigned long long cand = 0, mol = 0, rd = 0;
    for (uint64_t c = (uint64_t)blockIdx.x * CELLS_THREADS + threadIdx.x; c < n_cols; c += (uint64_t)gridDim.x * CELLS_THREADS) {
        const uint64_t t = cell_molecules[c];
        key[c] = t;
        val[c] = (uint32_t)c;
        cand += t != 0;
        mol += t;
        rd += cell_reads[c];
    }
    block_sum3(cand, mol, rd);
    if (threadIdx.x == 0) {
        if (cand) atomicAdd(ctl + CC_CANDIDATES, cand);
        if (mol) atomicAdd(ctl + CC_ALL_MOL, mol);
        if (rd) atomicAdd(ctl + CC_ALL_READS, rd);
    }
}

// pick: what min(n - 1, .) is taken of -- floor(N (1000 - P) / 1000) or N - 1 (the host's arithmetic)
__global__ __launch_bounds__(64) void cells_threshold_kernel(const uint64_t *__restrict__ sorted, uint32_t n_cols, int rule,
                                                             unsigned long long pick, unsigned long long ratio,
                                                             unsigned long long min_molecules, unsigned long long *ctl)
{
    if (threadIdx.x != 0) return;
    const unsigned long long n = ctl[CC_CANDIDATES];
    unsigned long long t = 0, m = 0;
    if (n != 0 && n <= n_cols) { // (n > n_cols: only where a column was counted twice, in an input that is refused)
        if (rule == CELLS_MIN) {
            t = std::max(1ull, min_molecules);
        } else {
            const unsigned long long i = std::min(n - 1ull, pick);
            const unsigned long long s = sorted[(unsigned long long)n_cols - 1ull - i];
            if (rule == CELLS_TOP) {
                t = s;
            } else { // s / ratio rounded half up; s < 2^62
                m = s;
                t = ratio > 2ull * m ? 1ull : std::max(1ull, (2ull * m + ratio) / (2ull * ratio));
            }
        }
    }
    ctl[CC_T] = t;
    ctl[CC_M] = m;
}

__global__ __launch_bounds__(CELLS_THREADS) void cells_call_kernel(const uint64_t *__restrict__ cell_molecules,
                                                                   const uint64_t *__restrict__ cell_reads,
                                                                   const uint32_t *__restrict__ cell_genes, uint32_t n_cols,
                                                                   uint8_t *__restrict__ called, uint64_t *__restrict__ flag,
                                                                   uint32_t *__restrict__ gene_key, uint32_t *__restrict__ gene_val,
                                                                   unsigned long long *ctl)
{
    const unsigned long long t = ctl[CC_T];
    unsigned long long mol = 0, rd = 0, unused = 0;
    for (uint64_t c = (uint64_t)blockIdx.x * CELLS_THREADS + threadIdx.x; c < n_cols; c += (uint64_t)gridDim.x * CELLS_THREADS) {
        const uint64_t tot = cell_molecules[c];
        const bool is = tot >= 1 && tot >= t;
        called[c] = is;
        flag[c] = is;
        gene_key[c] = is ? cell_genes[c] : 0u;
        gene_val[c] = (uint32_t)c;
        if (is) {
            mol += tot;
            rd += cell_reads[c];
        }
    }
    block_sum3(mol, rd, unused);
    if (threadIdx.x == 0) {
        if (mol) atomicAdd(ctl + CC_MOL, mol);
        if (rd) atomicAdd(ctl + CC_READS, rd);
    }
}

__global__ __launch_bounds__(CELLS_THREADS) void cells_number_kernel(const uint8_t *__restrict__ called, const uint64_t *__restrict__ incl,
                                                                     const uint64_t *__restrict__ sorted,
                                                                     const uint32_t *__restrict__ sorted_genes, uint32_t n_cols,
                                                                     uint32_t *__restrict__ new_col, unsigned long long *ctl)
{
    const uint64_t c = (uint64_t)blockIdx.x * CELLS_THREADS + threadIdx.x;
    if (c < n_cols) new_col[c] = called[c] ? (uint32_t)(incl[c] - 1ull) : 0xFFFFFFFFu;
    if (c == 0) {
        const unsigned long long k = incl[n_cols - 1];
        unsigned long long med_mol = 0, med_genes = 0;
        if (k) { // the called columns, ascending: the top k of either sort; the lower median among them
            const unsigned long long at = (unsigned long long)n_cols - k + (k - 1ull) / 2ull;
            med_mol = sorted[at];
            med_genes = sorted_genes[at];
        }
        ctl[CC_CALLED] = k;
        ctl[CC_MED_MOL] = med_mol;
        ctl[CC_MED_GENES] = med_genes;
    }
}

__global__ __launch_bounds__(CELLS_THREADS) void cells_flag_kernel(const uint32_t *__restrict__ col, const uint32_t *__restrict__ molecules,
                                                                   const uint8_t *__restrict__ called, uint32_t nnz, uint32_t n_cols,
                                                                   uint64_t *__restrict__ flag)
{
    const uint64_t i = (uint64_t)blockIdx.x * CELLS_THREADS + threadIdx.x;
    if (i >= nnz) return;
    const uint32_t c = col[i];
    flag[i] = c < n_cols && called[c] && molecules[i] != 0;
}

__global__ __launch_bounds__(CELLS_THREADS) void cells_scatter_kernel(const uint32_t *__restrict__ row, const uint32_t *__restrict__ col,
                                                                      const uint32_t *__restrict__ molecules,
                                                                      const uint64_t *__restrict__ reads, const uint64_t *__restrict__ flag,
                                                                      const uint64_t *__restrict__ incl, const uint32_t *__restrict__ new_col,
                                                                      uint32_t nnz, uint32_t *__restrict__ out_row,
                                                                      uint32_t *__restrict__ out_col, uint32_t *__restrict__ out_molecules,
                                                                      uint64_t *__restrict__ out_reads)
{
    const uint64_t i = (uint64_t)blockIdx.x * CELLS_THREADS + threadIdx.x;
    if (i >= nnz || !flag[i]) return; // (a flag is set for a column inside n_cols only)
    const uint64_t o = incl[i] - 1ull; // < nnz: the scan counts flags
    out_row[o] = row[i];
    out_col[o] = new_col[col[i]];
    out_molecules[o] = molecules[i];
    out_reads[o] = reads[i];
}

inline uint32_t blocks_for(uint64_t n, uint32_t per) { return (uint32_t)std::max<uint64_t>(1, (n + per - 1) / per); }

inline int bits_of(uint64_t v)
{
    int b = 0;
    while (b < 64 && (v >> b)) b++;
    return b;
}

} // namespace

size_t cells_workspace_bytes(uint32_t nnz, uint32_t n_cols) { return cells_carve(nullptr, nnz, n_cols).total; }

int call_cells_on_device(void *workspace, const CellsCall &c, hipStream_t s)
{
    const uint32_t nnz = c.nnz, n_cols = c.n_cols;
    const CellsWs w = cells_carve(workspace, nnz, n_cols);
    CELLS_TRY(hipMemsetAsync(w.ctl, 0, 256, s));
    CELLS_TRY(hipMemsetAsync(c.d_cell_molecules, 0, (size_t)n_cols * 8, s)); // (a run that crosses a block is added up in place)
    CELLS_TRY(hipMemsetAsync(c.d_cell_reads, 0, (size_t)n_cols * 8, s));
    CELLS_TRY(hipMemsetAsync(c.d_cell_genes, 0, (size_t)n_cols * 4, s));
    cells_sum_kernel<<<blocks_for(nnz, CELLS_SUM_THREADS), CELLS_SUM_THREADS, 0, s>>>(
        c.d_row, c.d_col, c.d_molecules, c.d_reads, nnz, c.n_rows, n_cols, (unsigned long long *)c.d_cell_molecules,
        (unsigned long long *)c.d_cell_reads, c.d_cell_genes, w.ctl);
    CELLS_TRY(hipGetLastError());
    const uint32_t col_blocks = std::min(blocks_for(n_cols, CELLS_THREADS), c.n_cus * 8);
    cells_keys_kernel<<<col_blocks, CELLS_THREADS, 0, s>>>(c.d_cell_molecules, c.d_cell_reads, n_cols, w.ka, w.va, w.ctl);
    CELLS_TRY(hipGetLastError());
    bool in_b = false;
    // (a total is below nnz * 2^32)
    CELLS_TRY(radix_sort_pairs_u64(w.ka, w.kb, w.va, w.vb, n_cols, 0, std::min(64, 32 + bits_of(nnz)), w.radix_tmp, w.radix_bytes,
                                   &in_b, s));
    const uint64_t *sorted = in_b ? w.kb : w.ka;
    uint64_t *flag = in_b ? w.ka : w.kb;
    cells_threshold_kernel<<<1, 64, 0, s>>>(sorted, n_cols, c.rule, c.pick, c.ratio, c.min_molecules, w.ctl);
    CELLS_TRY(hipGetLastError());
    cells_call_kernel<<<col_blocks, CELLS_THREADS, 0, s>>>(c.d_cell_molecules, c.d_cell_reads, c.d_cell_genes, n_cols, c.d_called, flag,
                                                          w.ga, w.va, w.ctl);
    CELLS_TRY(hipGetLastError());
    CELLS_TRY(scan_inclusive_u64(flag, w.incl, n_cols, w.scan_tmp, w.scan_bytes, s));
    bool g_in_b = false;
    // (a column has at most n_rows genes)
    CELLS_TRY(radix_sort_pairs_u32(w.ga, w.gb, w.va, w.vb, n_cols, 0, std::min(32, bits_of(c.n_rows)), w.radix_tmp, w.radix_bytes,
                                   &g_in_b, s));
    cells_number_kernel<<<blocks_for(n_cols, CELLS_THREADS), CELLS_THREADS, 0, s>>>(c.d_called, w.incl, sorted, g_in_b ? w.gb : w.ga,
                                                                                   n_cols, c.d_new_col, w.ctl);
    CELLS_TRY(hipGetLastError());
    cells_flag_kernel<<<blocks_for(nnz, CELLS_THREADS), CELLS_THREADS, 0, s>>>(c.d_col, c.d_molecules, c.d_called, nnz, n_cols, w.tflag);
    CELLS_TRY(hipGetLastError());
    CELLS_TRY(scan_inclusive_u64(w.tflag, w.tincl, nnz, w.scan_tmp, w.scan_bytes, s));
    cells_scatter_kernel<<<blocks_for(nnz, CELLS_THREADS), CELLS_THREADS, 0, s>>>(c.d_row, c.d_col, c.d_molecules, c.d_reads, w.tflag,
                                                                                w.tincl, c.d_new_col, nnz, c.d_out_row, c.d_out_col,
                                                                                c.d_out_molecules, c.d_out_reads);
    CELLS_TRY(hipGetLastError());
    CELLS_TRY(hipMemcpyAsync(c.h_pinned, w.ctl, CELLS_CTL_WORDS * 8, hipMemcpyDeviceToHost, s));
    CELLS_TRY(hipMemcpyAsync(c.h_pinned + CELLS_CTL_WORDS, w.tincl + (nnz - 1), 8, hipMemcpyDeviceToHost, s));
    CELLS_TRY(hipStreamSynchronize(s));
    return 0;
}

#undef CELLS_TRY

} // namespace umihip
