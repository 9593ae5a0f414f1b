/*
 * geglove.h -- C ABI of libgeglove.so, the MI355X (gfx950) implementation of the
 * Phaken/graph-embeddings hot path:  BCA co-occurrence builder  ->  GloVe/pGloVe
 * AdaGrad loop over the nonzero (i, j, X_ij) entries.
 *
 * The reference is pure Java with no native boundary; this header IS the
 * boundary a maintainer would bind over JNI (INTEGRATION.md shows the Java side).  Each
 * entry point cites the reference interface it replaces (J/ = src/main/java/org/uu/nl/embedding/).
 *
 * Conventions: plain C, no C++ types, no exceptions; every call returns ge_status
 * (0 = ok, <0 = error) and leaves a message readable through ge_last_error() (thread local).
 * The caller owns every host buffer passed in or filled; the library never keeps a host
 * pointer after the call returns.  Handles are opaque and freed only by *_destroy.
 * Calls on one handle are blocking and not re-entrant; distinct handles are independent.
 * The library never calls exit()/abort().  There is NO CPU fallback: every entry point
 * that computes needs a gfx950 device and fails with GE_ERR_HIP otherwise.
 */
#ifndef GEGLOVE_H
#define GEGLOVE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t ge_status;
enum {
    GE_OK           =  0,
    GE_ERR_ARG      = -1,   /* invalid argument (the Java path throws IllegalArgumentException / InvalidConfigurationException) */
    GE_ERR_OOM      = -2,   /* host or device allocation failed */
    GE_ERR_HIP      = -3,   /* HIP runtime error / no device */
    GE_ERR_STATE    = -4,   /* call not valid in the handle's current state */
    GE_ERR_OVERFLOW = -5    /* a per-bookmark work buffer overflowed (BCA frontier / row capacity) */
};

/* Configuration.EmbeddingMethod (J/util/config/Configuration.java:19-21): picks
 * GloveCost (J/opt/GloveCost.java:5-21) or PGloveCost (J/opt/PGloveCost.java:5-21). */
enum { GE_COST_GLOVE = 0, GE_COST_PGLOVE = 1 };
/* Configuration.OptimizationMethod (J/util/config/Configuration.java:23-25); Main.createOptimizer
 * (J/Main.java:121-130): Adagrad (J/opt/grad/Adagrad.java), Adam (J/opt/grad/Adam.java:75-147),
 * AMSGrad (J/opt/grad/AMSGrad.java:91-162).  beta1 = 0.9f, beta2 = 0.999f, epsilon = 1e-7f as hard coded there. */
enum { GE_OPT_ADAGRAD = 0, GE_OPT_ADAM = 1, GE_OPT_AMSGRAD = 2 };
/* Configuration.BCANormalization (J/util/config/Configuration.java:31-33). */
enum { GE_NORM_NONE = 0, GE_NORM_UNITY = 1, GE_NORM_COUNTS = 2 };

/* How the update loop is scheduled on the device.
 * DETERMINISTIC: the exact semantics of the Java loop with `threads: T` where the T jobs of
 *   Adagrad.createJob (J/opt/grad/Adagrad.java:42-98) run one after another in id order;
 *   for T = 1 this IS the Java result, bit for bit (sequential fp32 dot, fp64 sqrt/div as in
 *   :76-77, :88-89).  One wavefront; a parity / reproducibility mode, not a fast one.
 * HOGWILD: the production mode.  Thousands of lane groups update the shared tables without
 *   locks, exactly as the Java worker threads do (J/opt/Optimizer.java:27-28 are plain arrays),
 *   fp32 arithmetic, wave-reduced dot.
 * STRATIFIED: DETERMINISTIC's arithmetic, operation for operation, on P wavefronts at once and still a function of the input
 *   alone: same bytes run after run, machine after machine, no update lost.  Product semantics (the reference has no counterpart):
 *   notation   N = nnz, nonzero k = (I[k], J[k], X[k]) in matrix order, P = the number of strata (below).
 *   partition  r(i) = #{k : I[k] < i},  c(j) = #{k : J[k] < j};  rb(i) = (r(i) * P) / N,  cb(j) = (c(j) * P) / N  (64-bit integer
 *              division): P row blocks and P column blocks, contiguous id ranges balanced by nonzero count; empty blocks are legal.
 *              Tile (a, b), id T = a * P + b, holds the nonzeros with rb(I[k]) = a and cb(J[k]) = b in ascending k; n_T of them.
 *   schedule   sub-epoch s = the P tiles (a, (a + s) mod P), a = 0 .. P-1.  They share no focus row and no context row, so they
 *              run concurrently (one wavefront each) without touching a common table row, and the tables end up, bit for bit, as
 *              if the tiles had run one after another.  Sub-epochs are separate kernel launches: nothing else synchronises.
 *   order      GE_SHUFFLE_NONE: sub-epochs s = 0 .. P-1, each tile in ascending k.  GE_SHUFFLE_DEVICE: the t-th sub-epoch run
 *              is s = B(P, K(0))(t), and the q-th update of tile T is its B(n_T, K(T + 1))(q)-th nonzero, where
 *                B(n, key)(x): b = the smallest b >= 0 with 2^b >= n, m = 2^b - 1, sh = b > 1 ? b / 2 : 1;  y = x;
 *                              repeat  y = R(y)  until y < n;   R(y): for q = 0 .. 3 { y = (y + key[q]) & m;  y = (y * C[q]) & m;
 *                              y ^= y >> sh },  C = { 0x9E3779B1, 0x85EBCA6B, 0xC2B2AE35, 0x27D4EB2F }  (32-bit unsigned);
 *                K(salt):      z = seed * 0x9E3779B97F4A7C15 + (uint32) iteration * 0xD1B54A32D192ED03 + 0x632BE59BD9B4E019
 *                              + salt * 0xA0761D6478BD642F  (mod 2^64);  for q = 0 .. 3 { z += 0x9E3779B97F4A7C15;  t = z;
 *                              t = (t ^ (t >> 30)) * 0xBF58476D1CE4E5B9;  t = (t ^ (t >> 27)) * 0x94D049BB133111EB;
 *                              t ^= t >> 31;  key[q] = the low 32 bits of t }.
 *              GE_SHUFFLE_JAVA is GE_ERR_ARG: a global Fisher-Yates order cannot be stratified.
 *              ge_glove_epoch_order returns the sequential equivalent: sub-epochs in the order they run, inside a sub-epoch
 *              a ascending, inside a tile its walk.
 *   cost       every tile is a job with its own fp32 accumulator starting at 0 (Adagrad.java:60); *cost_sum = the fp64 sum of
 *              the tile costs in that same order.
 *   P          cfg.strata, 1 <= P <= 2048; 0 = the largest power of two P with 8 * P * P <= N and P <= owned rows (at least 1,
 *              at most 2048): a function of (rows, nnz) alone, never of the device.  A nonzero cfg.strata with another mode
 *              is GE_ERR_ARG.
 *   bound      an epoch takes ge_glove_info.strata_path = sum_s max_a n_(a, (a + s) mod P) sequential updates.  That is at least
 *              the busiest row block and the busiest column block, and a single column with more than N / P nonzeros sets the
 *              floor by itself, whatever P: 7.7 % of N on the 300-vertex Zipf test matrix, 1.0 % on the 100 k-vertex one (C2),
 *              under 0.1 % on BCA-built matrices.  An epoch is at most P kernel launches (a sub-epoch without a nonzero is not
 *              launched); measured: DESIGN.md 3.7.
 *   fp32 rows only (bf16 is GE_ERR_ARG), plain tables as for DETERMINISTIC handles; threads, workers, the hub and the layout
 *   fields are ignored; row_begin / row_end as for DETERMINISTIC (r and c count this handle's nonzeros). */
enum { GE_MODE_HOGWILD = 0, GE_MODE_DETERMINISTIC = 1, GE_MODE_STRATIFIED = 2 };

/* The arithmetic of one update of a GE_MODE_STRATIFIED handle (ge_glove_set_arith).  The schedule, the order and every guarantee
 * of the mode are the same for both: race-free, bytes a function of (input, seed, P) alone, the sequential equivalent that
 * ge_glove_epoch_order reports.
 * JAVA (the default): DETERMINISTIC's arithmetic, as stated above.
 * FP32: for nonzero (i, j, x) of a tile, a = focus[i], b = context[j], D = dim.  Every operation is an IEEE fp32 operation,
 *   rounded to nearest even, unless marked fp64; nothing is contracted beyond the fmas named here.
 *   lane shape  the Hogwild one: vw = 4 if D % 4 == 0, else 2 if D % 2 == 0, else 1; nch = ceil(D / (64 * vw)); lane L of 64 holds
 *               elements [vw * (L + 64 q), + vw) of chunk q < nch.  nch > 4 has no kernel (ge_glove_set_arith: GE_ERR_ARG).
 *   dot         per lane  part = 0;  for q = 0 .. nch-1, t = 0 .. vw-1:  part = fmaf(a[e], b[e], part)  with e = vw * (L + 64 q) + t
 *               (an element past the row contributes nothing).  Then the tree: in each row of 16 lanes  v[L] += v[L ^ 1];
 *               v[L] += v[L ^ 2];  v[L] += v[(L & ~7) | (7 - (L & 7))];  v[L] += v[(L & ~15) | (15 - (L & 15))];  and
 *               dot = (v[0] + v[16]) + (v[32] + v[48]).
 *   cost terms  GloVe: l = log((double) x) (fp64), w = x > xmax ? 1 : (float) pow((double) x / xmax, 0.75) (fp64 libm pow);
 *               pGloVe: l = log((double) (x / (1.0f - x))), w = x: DETERMINISTIC's.  Computed once per nonzero on the first
 *               switch to FP32 (12 bytes per nonzero).
 *   ic, wc      ic = (float) ((double) dot + ((double) (fbias[i] + cbias[j]) - l));  wc = w * ic.
 *   tile cost   cost = (float) ((double) cost + (0.5 * (double) wc) * (double) ic) from 0 per tile; *cost_sum as above.
 *   AdaGrad     per element, g1 = wc * b, g2 = wc * a from the values read before either row changes:
 *               a' = a - (g1 / sqrtf(Ga)) * lr,  b' = b - (g2 / sqrtf(Gb)) * lr,  Ga' = Ga + g1 * g1,  Gb' = Gb + g2 * g2;
 *               fbias' = fbias - wc / sqrtf(Gfb),  Gfb' = Gfb + wc * wc, and the same for cbias: Adagrad.java's expression
 *               order with every operation in fp32.  sqrtf and / are correctly rounded.
 *   Adam / AMSGrad  HOGWILD's: m' = fmaf(0.9f, m, (1 - 0.9f) * g);  vn = fmaf(0.999f, v, (1 - 0.999f) * (g * g));
 *               v' = AMSGrad ? max(v, vn) : vn;  par' = par - corr * m' * (1.0f / (sqrtf(v') + 1e-7f))  (left to right), with
 *               corr = Adam ? (float) (lr * sqrt(1 - beta2^(t+1)) / (1 - beta1^(t+1))) (fp64, Adam.java:84) : lr;  the context
 *               row takes g = g2, the focus row g = g1, the biases g = wc.
 *   Switching between epochs is legal: both arithmetics work on the same plain fp32 tables. */
enum { GE_ARITH_JAVA = 0, GE_ARITH_FP32 = 1 };

/* Order in which an epoch visits the nonzeros.
 * JAVA:   CoOccurrenceMatrix.shuffle() = cumulative forward Fisher-Yates on one permutation,
 *         drawn from the SAME java.util.Random stream that initialised the parameters
 *         (J/opt/Optimizer.java:79; J/util/rnd/Permutation.java:21; ExtendedRandom.java:398-407).
 * DEVICE: (HOGWILD) the matrix is cut once into chunks of 128 nonzeros -- hub columns column-major, the
 *         rest row-major as BookmarkColoring emits it -- and every epoch visits the chunks in a fresh
 *         keyed-bijection order evaluated inside the kernel (no permutation array, no host work).  One
 *         side of each update then stays in registers for a whole run, which halves the HBM traffic.
 *         Not the Java order; measured statistically equivalent.  (DETERMINISTIC: a keyed
 *         bijection of the nonzeros themselves.)
 * NONE:   matrix order (no shuffle). */
enum { GE_SHUFFLE_JAVA = 0, GE_SHUFFLE_DEVICE = 1, GE_SHUFFLE_NONE = 2 };

/* Lock-free does not mean lossy on a GPU: ~10^4 lane groups are in flight (the JVM has <= #cores
 * threads), so a hub column j that appears in a large share of the nonzeros would lose most of its
 * concurrent plain read-modify-write updates.  Nonzeros of such "hot" columns therefore update the
 * context side with float atomic adds (no update is lost; gradients may be a few microseconds
 * stale, as under Hogwild) and read it with agent-coherent loads.
 * AUTO: column j is hot when  count(j) * groups_in_flight >= 0.25 * N  (library default).
 * NONE: no column is treated as a hub: context rows are always read, updated and stored plainly (the literal Java race on that
 *   side; focus rows are still never overwritten, see GE_LAYOUT_*).  ALL: every column (tests). */
enum { GE_HOT_AUTO = 0, GE_HOT_NONE = 1, GE_HOT_ALL = 2 };

/* Storage type of the embedding rows (focus, context).  BF16 is BASELINE config C5: bf16 rows, fp32 AdaGrad
 * accumulators and biases, fp32 arithmetic; rows are narrowed with stochastic rounding, hub context rows keep an
 * fp32 master copy.  HOGWILD + GE_SHUFFLE_DEVICE + ADAGRAD + dim % 4 == 0 only (the reference is fp32 throughout,
 * so there is no bit-exact mode for it); every API still speaks fp32 (get/set/extract convert). */
enum { GE_DTYPE_F32 = 0, GE_DTYPE_BF16 = 1 };

/* Parameter tables a caller can read or write (tests, checkpointing, multi-GPU sync). */
enum {
    GE_STATE_FOCUS = 0,        /* float[V*D]  Optimizer.focus         (J/opt/Optimizer.java:27) */
    GE_STATE_CONTEXT = 1,      /* float[V*D]  Optimizer.context                                  */
    GE_STATE_FBIAS = 2,        /* float[V]    Optimizer.fBias         (J/opt/Optimizer.java:28) */
    GE_STATE_CBIAS = 3,        /* float[V]    Optimizer.cBias                                    */
    GE_STATE_GSQ_FOCUS = 4,    /* float[V*D]  Adagrad.gradSqFocus     (J/opt/grad/Adagrad.java:16) | Adam/AMSGrad.M1focus   */
    GE_STATE_GSQ_CONTEXT = 5,  /* float[V*D]  Adagrad.gradSqContext                                | Adam/AMSGrad.M1context */
    GE_STATE_GSQ_FBIAS = 6,    /* float[V]    Adagrad.gradSqFBias     (J/opt/grad/Adagrad.java:17) | Adam/AMSGrad.M1fBias   */
    GE_STATE_GSQ_CBIAS = 7,    /* float[V]    Adagrad.gradSqCBias                                  | Adam/AMSGrad.M1cBias   */
    GE_STATE_M2_FOCUS = 8,     /* float[V*D]  Adam/AMSGrad.M2focus    (J/opt/grad/Adam.java:40-41); empty for Adagrad */
    GE_STATE_M2_CONTEXT = 9,   /* float[V*D]  Adam/AMSGrad.M2context */
    GE_STATE_M2_FBIAS = 10,    /* float[V]    Adam/AMSGrad.M2fBias   */
    GE_STATE_M2_CBIAS = 11,    /* float[V]    Adam/AMSGrad.M2cBias   */
    GE_STATE_COUNT = 12
};

/* ------------------------------------------------------------------------------------------
 * Trainer.  Replaces `new Adagrad(coMatrix, config, costFunction)` + IOptimizer
 * (J/opt/IOptimizer.java:6-11; J/opt/Optimizer.java:34-64; J/opt/grad/Adagrad.java:19-34).
 * ---------------------------------------------------------------------------------------- */
typedef struct ge_glove ge_glove;

typedef struct {
    int32_t vocab_size;     /* V = coMatrix.vocabSize()          (J/opt/Optimizer.java:40)            */
    int32_t dim;            /* D = config.getDim()               (J/opt/Optimizer.java:43); V*D < 2^31 as in Java */
    int64_t nnz;            /* N = coMatrix.coOccurrenceCount()  (J/opt/Optimizer.java:42); N < 2^31 as in Java  */
    int32_t cost;           /* GE_COST_*                                                               */
    int32_t opt;            /* GE_OPT_*                                                                */
    float   learning_rate;  /* 0.05f in the reference, hard coded (J/opt/Optimizer.java:26)            */
    double  xmax;           /* coMatrix.max()                    (J/opt/GloveCost.java:19)             */
    int64_t seed;           /* Configuration.setThreadLocalRandom(seed) (J/util/config/Configuration.java:161-163) */
    int32_t threads;        /* config.getThreads(): job slicing N/T (+N%T on the last), J/opt/Optimizer.java:59-63.
                               Used by DETERMINISTIC mode only; HOGWILD ignores it.  >= 1.             */
    int32_t mode;           /* GE_MODE_*                                                               */
    int32_t shuffle;        /* GE_SHUFFLE_*                                                            */
    int32_t device;         /* HIP device ordinal                                                      */
    void   *stream;         /* hipStream_t to launch on, or NULL for the device's null stream          */
    int32_t row_begin;      /* multi-GPU row sharding: this handle owns focus rows      */
    int32_t row_end;        /*   [row_begin,row_end); 0,0 = all rows.  I[] must lie inside the range.  */
    int32_t hot_columns;    /* GE_HOT_* (HOGWILD mode only)                                            */
    int32_t workers;        /* HOGWILD: number of sequential workers (wavefronts); 0 = fill the device.
                               Workers pull chunks of 128 consecutive nonzeros of the epoch order from a queue
                               and walk each chunk in stable column order; workers = 1 is fully sequential, for any
                               flush limit: a cut hub run continues from what it has just published
                               (tests/test_designed_matrices_gpu.py replays it with flush_every 1, 3, 4, 64).
                               workers = -k fills the device except for k wavefront slots, which stay free for
                               kernels running beside the epoch (the all-reduce of an overlapped exchange). */
    int32_t emb_dtype;      /* GE_DTYPE_*: storage of the focus/context rows                           */
    /* HOGWILD tuning; 0 = the library default everywhere.  These change results (which columns publish by delta,
     * how stale a hub run may get), so they live here and under the YAML `device:` block, not in the environment. */
    float   hot_theta;      /* GE_HOT_AUTO: column j is a hub when count(j) * workers >= hot_theta * N.  Default 0.25 */
    float   stale_budget;   /* a hub run is cut (delta published, row re-read behind the publish) every m_j updates with
                               K_j * m_j <= stale_budget, K_j = expected workers inside column j.  Default 2000
                               (measured: 10 000 is stable at the bench scale, 39 000 diverges)                */
    int32_t flush_every;    /* > 0: cut every hub run after this many updates instead (<= 128)              */
    int32_t blocks_per_cu;  /* > 0: workgroups of 4 workers per CU; default = what the occupancy API reports */
    int32_t layout_flags;   /* GE_LAYOUT_* below                                                            */
    int32_t strata;         /* GE_MODE_STRATIFIED: P, 1 .. 2048; 0 = the default for (rows, nnz).  Must be 0 in every other mode */
} ge_glove_cfg;

/* ge_glove_cfg.layout_flags (GE_SHUFFLE_DEVICE handles).  Default 0: focus rows are packed whole into chunks, so a row
 * is resident in one worker per epoch; a row with more than 128 ordinary nonzeros is cut into pieces that publish the row
 * by delta (float atomics; bf16 rows and Adam/AMSGrad: re-read + add + store), so no worker overwrites another one's run.
 * FIXED_CUTS     round-1 layout: chunks cut every 128 positions whatever the rows (a row cut by a chunk boundary can be
 *                resident in two workers; the later store discards the other worker's whole run) -- ablation / tests.
 * PLAIN_LONG_ROWS  pieces of long rows store plainly (same hazard for those rows only) -- ablation / tests.
 * SEPARATE_TABLES  round-1 storage: a table per kind.  Default (fp32 rows): a side's row and its accumulator row (and
 *                second-moment row) are ONE record of 2 (3) x row width floats, so the loads / stores of one update touch
 *                one region per side instead of two -- measured 7 % faster in alternation and free of the slow placements
 *                separate tables fall into -- ablation / tests.
 * PACKED_RECORDS  fat rows exactly dim + 4 floats wide and records back to back, as before the alignment work.  Default:
 *                records start on 64-byte boundaries, and an fp32 row with dim % 4 == 0 is as wide as the whole 64-byte lines
 *                that hold dim + 1 floats (dim 200: 208; skipped where that would add more than 10 %), so every row store writes
 *                whole lines and a row shares no line with its accumulator row -- ablation / tests.
 * FIRST_PLACEMENT  take the record tables where the first allocation puts them.  Default: each side's table is allocated up to six
 *                times (the earlier ones held meanwhile), a millisecond of random record reads and write-backs is timed on each, the
 *                fastest is kept and the others freed -- where the driver places a table decides which of two epoch times a handle
 *                gets (same process, same virtual address, 48 or 54 ms) -- ablation / tests.
 * HUB_TILES      hub tiles for every group of >= 2 hub columns, whatever the matrix's size and the columns' density -- tests, small
 *                matrices: the build keeps a counter per (group, focus row) and a 32-bit sort key per (group, row, slot); a matrix
 *                with more than 2^28 (group, row) pairs, or too many for the key, is refused with GE_ERR_ARG under this flag (by
 *                default such a handle builds no tiles, and ge_glove_tile_info says so with zeros).
 *                Hub tiles: the densest hub columns are walked in groups of 4 that stay resident in a worker while
 *                each focus row streams through once per group instead of once per nonzero.  Default: columns with
 *                count >= rows / 8, on fp32 AdaGrad handles with dim % 4 == 0, dim <= 252, that own every focus row and hold
 *                >= 2^25 nonzeros; every other handle keeps its chunk table and its kernel.  Ignored where the handle's kernel
 *                has no tile walk (bf16 rows, Adam / AMSGrad, other dims, shards).
 * NO_HUB_TILES   never build hub tiles (wins over HUB_TILES).
 * HUB_PANELS     hub panels: four consecutive full groups of tile columns form a panel; the four wavefronts of a
 *                workgroup hold one group each and pass every focus row of a panel chunk from one to the next, so the row streams
 *                once per 16 columns; groups that fill no panel stay tiles.  Default: handles that build hub tiles by default (>= 2^25
 *                nonzeros).  Under this flag a smaller handle builds its panels from forced tiles, as under HUB_TILES (tests, small
 *                matrices).
 * NO_HUB_PANELS  never build hub panels (wins over HUB_PANELS and DEEP_PANELS): the handle's layout, kernel and results are those of a
 *                library without panels.
 * DEEP_PANELS    hub panels walked by the ring kernel: stage 0 of the panel pipeline keeps the focus pairs of
 *                several rows in flight instead of one.  Forces panels at any size as HUB_PANELS does (a handle below 2^25 nonzeros
 *                builds them from forced tiles, every hub column eligible); the same layout, the same sequential program.  Default:
 *                handles that build hub panels by default, unless HUB_PANELS is set -- a HUB_PANELS handle without this flag keeps
 *                the one-row-ahead kernel.
 * NO_DEEP_PANELS never run the ring kernel (wins over DEEP_PANELS and over the default): the handle's layout, kernel and results are
 *                those of a library without it.
 * DEEP_WALK      the ring kernel with the ordinary walk two nonzeros deep: a worker keeps the streamed pairs of
 *                the next two nonzeros in flight instead of one.  Forces what DEEP_PANELS forces; the same layout, the same
 *                sequential program.  Never the default: at the bench size it is no faster than the ring kernel and the racing
 *                workers end at a higher cost -- experiments and tests.
 * NO_DEEP_WALK   never run the depth-2 walk (wins over DEEP_WALK): the handle's layout, kernel and results are those of a library
 *                without it. */
enum { GE_LAYOUT_FIXED_CUTS = 1, GE_LAYOUT_PLAIN_LONG_ROWS = 2, GE_LAYOUT_SEPARATE_TABLES = 4, GE_LAYOUT_PACKED_RECORDS = 8, GE_LAYOUT_FIRST_PLACEMENT = 16,
       GE_LAYOUT_HUB_TILES = 32, GE_LAYOUT_NO_HUB_TILES = 64, GE_LAYOUT_HUB_PANELS = 128, GE_LAYOUT_NO_HUB_PANELS = 256,
       GE_LAYOUT_DEEP_PANELS = 512, GE_LAYOUT_NO_DEEP_PANELS = 1024, GE_LAYOUT_DEEP_WALK = 2048, GE_LAYOUT_NO_DEEP_WALK = 4096 };

/* What the library decided for a handle (reporting / DESIGN.md numbers). */
typedef struct {
    int32_t group_width;      /* lanes that own one nonzero (16, 32 or 64)                 */
    int32_t vector_width;     /* floats per lane access (4, 2 or 1)                        */
    int32_t chunks_per_lane;
    int32_t blocks;           /* workgroups launched per epoch                             */
    int32_t groups_in_flight; /* sequential workers (wavefronts) in flight                 */
    int32_t hot_columns;      /* columns updated with atomics                              */
    int64_t hot_nonzeros;     /* nonzeros whose column is hot                              */
    int64_t hot_threshold;    /* count(j) >= this => hot                                   */
    int64_t chunks;           /* GE_SHUFFLE_DEVICE: chunks per epoch (<= 128 nonzeros each) ...          */
    int64_t hub_chunks;       /*   ... of which hub-column chunks                                         */
    int64_t long_rows;        /*   focus rows cut into pieces (more than 128 ordinary nonzeros)           */
    int64_t shared_chunks;    /*   chunks that are such a piece (they publish the row by delta)           */
    int32_t flush_min;        /* smallest flush limit of a hub run                                        */
    int32_t row_stride;       /* floats between rows of the fp32 row tables                               */
    int64_t runs;             /*   runs per epoch: a run loads its resident row pair once and publishes it once */
    int64_t schedule_bytes;   /* bytes one epoch of this schedule has to move (what bench.py's roofline.achieved divides by the
                                 kernel time): per nonzero 20 B of (bA, bB, L, W) + the streamed row and its accumulator row(s)
                                 loaded and stored; per run the resident row and its accumulator row(s) loaded and published */
    int32_t placements;       /* allocations tried for the record tables, both sides together (2 = no choice was made)              */
    float   placement_best_ms, placement_worst_ms;   /* probe times of the kept and of the slowest candidate, summed over the two sides */
    int32_t reserved_;
    int32_t strata;           /* GE_MODE_STRATIFIED: the P in use (0 for the other modes)                                          */
    int64_t strata_path;      /*   sum over sub-epochs of the largest tile: the epoch's length in sequential updates               */
} ge_glove_info;


/* Fills *cfg with the reference's defaults (adagrad, lr 0.05f, threads 1, HOGWILD, DEVICE shuffle). */
void ge_glove_cfg_default(ge_glove_cfg *cfg);

/* I, J, X: host arrays of length cfg->nnz in matrix (pre-shuffle) order, i.e. what
 * cIdx_I/J/C(k) return before the first shuffle() (J/util/CoOccurrenceMatrix.java:12-14).
 * Initialises focus/context/biases from java.util.Random(seed) in the reference's draw order
 * (J/opt/Optimizer.java:50-57), gradSq* = 1 (J/opt/grad/Adagrad.java:27-33), identity permutation. */
ge_status ge_glove_create(const ge_glove_cfg *cfg,
                          const int32_t *I, const int32_t *J, const float *X,
                          ge_glove **out);

/* One pass of the body of Optimizer.optimize()'s loop (J/opt/Optimizer.java:79-94):
 * shuffle, run all jobs, *cost_sum = sum over jobs of the job cost (what `localCost` holds at
 * :94, BEFORE the division by coCount at :96).  `iteration` mirrors createJob's argument
 * (unused by AdaGrad; it keys the DEVICE shuffle). */
ge_status ge_glove_epoch(ge_glove *h, int32_t iteration, double *cost_sum);

/* Optimizer.extractResult (J/opt/Optimizer.java:129-140): out[k] = (focus[k]+context[k])/2.
 * _f32 keeps fp32; _f64 widens as the Java double[] does. out has V*D elements (row-major). */
ge_status ge_glove_extract_f32(ge_glove *h, float *out);
ge_status ge_glove_extract_f64(ge_glove *h, double *out);

/* Copy one GE_STATE_* table device->host / host->device (count = number of floats). */
ge_status ge_glove_get_state(ge_glove *h, int32_t which, float *out, int64_t count);
ge_status ge_glove_set_state(ge_glove *h, int32_t which, const float *in, int64_t count);
/* Raw device pointer of a table (for zero-copy wrapping by the host runtime, e.g. the
 * torch.distributed/RCCL all-reduce of the context factors). Valid until destroy.
 * GE_MODE_DETERMINISTIC handles: the table as the API shows it, *count floats.  GE_MODE_HOGWILD handles with fp32 rows keep
 * FAT rows (a row's bias at [dim]; row width dim + 4 or the whole lines that hold it) inside records of ge_context_layout.row_stride floats (row | accumulator
 * row | ...): a row table id returns the address of ITS row in the first record and *count = the floats from there to the end
 * of its row in the last record; a bias table id returns the address of row 0's scalar inside the row that carries it (FBIAS ->
 * column [dim] of FOCUS, GSQ_CBIAS -> column [dim] of GSQ_CONTEXT ...; with bf16 rows both scalars follow the accumulator row:
 * GSQ_*BIAS at its column [dim], *BIAS at [dim + 1]), the scalar of row r being element r * row_stride from there (row_stride:
 * ge_glove_info.row_stride floats).  bf16 row tables are refused (ge_glove_context_layout). */
ge_status ge_glove_device_ptr(ge_glove *h, int32_t which, void **dptr, int64_t *count);

/* GE_MODE_STRATIFIED handles: the sequential order the epoch equals (see GE_MODE_STRATIFIED).
 * The order in which ONE worker (cfg.workers = 1) walks the nonzeros in epoch `iteration` of a HOGWILD handle:
 * out[k] = index into the caller's I/J/X of the k-th update.  With more workers the same chunks of 128 are
 * handed out in this order but run concurrently.  (GE_SHUFFLE_JAVA: the order of the most recent epoch.)
 * Lets a sequential implementation replay the device pass exactly (parity tests). */
ge_status ge_glove_epoch_order(ge_glove *h, int32_t iteration, int32_t *out, int64_t count);

/* Current permutation (GE_SHUFFLE_JAVA only) and java.util.Random state, for parity tests. */
ge_status ge_glove_get_perm(ge_glove *h, int32_t *out, int64_t count);
ge_status ge_glove_rng_state(ge_glove *h, uint64_t *state);

/* Device time of the last epoch's update kernel(s), measured with hipEvents on the launch
 * stream, in milliseconds; *launches = number of kernel launches it covered. */
ge_status ge_glove_last_kernel_ms(ge_glove *h, float *ms, int32_t *launches);

ge_status ge_glove_get_info(ge_glove *h, ge_glove_info *info);

/* The hub tiles of a handle's layout (GE_LAYOUT_HUB_TILES): out = [tile chunks, nonzeros inside them, columns per group, columns in
 * tiles]; all zero for a handle without tiles.  ge_glove_info.chunks includes the tile chunks, hub_chunks stays the column-major ones. */
ge_status ge_glove_tile_info(ge_glove *h, int64_t out[4]);

/* The hub panels of a handle's layout (GE_LAYOUT_HUB_PANELS): out = [panel chunks, nonzeros inside them, columns in panels, workgroups
 * that start in the panel loop]; all zero for a handle without panels.  The panel chunks have a queue of their own: they are no part
 * of ge_glove_info.chunks, and ge_glove_tile_info counts only what stayed tiles.  ge_glove_epoch_order lists them first. */
ge_status ge_glove_panel_info(ge_glove *h, int64_t out[4]);

/* GE_MODE_STRATIFIED handles: choose the arithmetic of the following epochs (GE_ARITH_*; JAVA after create).  A NULL handle or an
 * unknown value is GE_ERR_ARG, a handle of another mode GE_ERR_STATE, GE_ARITH_FP32 with a dim that has no lane shape GE_ERR_ARG.
 * ge_glove_cfg and ge_glove_info do not carry it. */
ge_status ge_glove_set_arith(ge_glove *h, int32_t arith);
ge_status ge_glove_get_arith(const ge_glove *h, int32_t *arith);

void ge_glove_destroy(ge_glove *h);

/* ------------------------------------------------------------------------------------------
 * Co-occurrence builder.  Replaces `new BookmarkColoring(graph, config)`
 * (J/bca/BookmarkColoring.java:32-120) once the host has flattened the grph graph into
 * weighted CSR (out-neighbours) + CSC (in-neighbours), which is what
 * In/OutEdgeNeighborhoodAlgorithm.compute + getIn/OutNeighborhoods produce
 * (J/bca/BookmarkColoring.java:49-52; J/convert/util/EdgeNeighborhoodAlgorithm.java:22-33).
 * ---------------------------------------------------------------------------------------- */
typedef struct ge_coo ge_coo;

typedef struct {
    int32_t        num_vertices;   /* V */
    const int64_t *ptr;            /* V+1 offsets */
    const int32_t *idx;            /* neighbour ids, unique within a row, in grph neighbour order */
    const float   *weight;         /* edge weight per neighbour (NumericalProperty.getValueAsFloat) */
} ge_csr;

typedef struct {
    double  alpha;       /* bca.alpha   (J/util/config/Configuration.java:322) */
    double  epsilon;     /* bca.epsilon */
    int32_t directed;    /* bca.directed: 1 = DirectedWeighted (forward + forced reverse pass), 0 = UndirectedWeighted */
    int32_t normalize;   /* GE_NORM_* */
    int32_t device;      /* HIP device ordinal */
    int32_t row_begin;   /* bookmarks [row_begin,row_end) only; 0,0 = all (multi-GPU sharding) */
    int32_t row_end;
    int64_t table_slots; /* sizing only, results do not depend on it: slots of a wavefront's work table (0 = from V; it
                            grows by itself on overflow) ...                                                       */
    int64_t pool_entries;/*   ... and entries of the first row pool (0 = from a sample of 2048 bookmarks)            */
} ge_bca_cfg;
/* Diagnostics read from the environment (never results): GE_BCA_TIMING=1 prints the phases of ge_bca_build to stderr. */

/* Runs one BCA job per bookmark (BCAJob.call, J/bca/util/BCAJob.java:31-36) on the device and
 * assembles the COO in ascending bookmark order with each row in java.util.HashMap iteration
 * order -- the order BookmarkColoring produces with `threads: 1`. */
ge_status ge_bca_build(const ge_csr *out_nbrs, const ge_csr *in_nbrs, const ge_bca_cfg *cfg, ge_coo **result);

/* Host views into the result (owned by the handle, valid until ge_coo_destroy):
 * I/J/X = coOccurrenceIdx_I/_J/Values (J/bca/BookmarkColoring.java:23-25), *max = max() (:153),
 * row_ptr[V+1] = first entry of each bookmark.  Any out pointer may be NULL. */
ge_status ge_coo_get(const ge_coo *c, int64_t *nnz, const int32_t **I, const int32_t **J,
                     const float **X, const int64_t **row_ptr, double *max);
void ge_coo_destroy(ge_coo *c);

/* ------------------------------------------------------------------------------------------
 * Synthetic co-occurrence matrix, generated on the device ("generated per-shard on device, seed 0xC0FFEE +
 * gpu"), and a trainer that reads it in place.  The reference has no generator, so these are product semantics.  The recipe is
 * integer and bit operations only: tests/synth_ref.py is the same recipe in numpy and holds the device output to the last bit.
 * (geglove/synth.py's host recipe goes through fp64 pow and stays what bench.py uses.)
 *   notation  SM(s, n) = the (n+1)-th SplitMix64 output of seed s;  hi(u) = u >> 32;  lo(u) = u & 0xFFFFFFFF.
 *   relabel   the stable argsort of SM(seed ^ 0x77777777, 0 .. V-1): a function of the seed alone, so every shard of one
 *             matrix sees the same hub columns.
 *   stream    s = (seed + 0x1000003 * (row_begin + 1)) mod 2^64;  rows = row_end - row_begin.
 *   draw t    a = SM(s, t), b = SM(s ^ 0x5A5A5A5A, t), c = SM(s ^ 0x0F0F0F0F, t)   for t = 0, 1, ...
 *     row     i = row_begin + ((hi(a) * rows) >> 32)
 *     rank    B = bit_length(V);  k = (hi(b) * B) >> 32;  r = 2^k - 1 + (lo(b) >> (32 - k)), r = 0 for k = 0: octave k has
 *             mass 1 / B over 2^k ranks, a density proportional to 1 / rank.
 *     void    when r >= V or relabel[r] == i; else j = relabel[r].
 *     value   e = 3 + ((hi(c) * 10) >> 32);  x = the fp32 with bits ((127 - e) << 23) | (c & 0x7FFFFF), then min(x, 0.2f):
 *             0 < x <= 0.2, pGloVe-valid.
 *   result    the diagonal (i, i, 0.2f) of the owned rows plus the first M = nnz - rows distinct valid keys (i, j) in ascending
 *             t, each with the x of its first occurrence; sorted by (i, j); exactly nnz entries.  A function of the arguments
 *             alone: not of the ranges the draws were taken in, nor of the machine.  No floating-point atomics.
 *   budget    8 * M + 1024 draws; a request that does not reach M distinct keys within it is GE_ERR_ARG ("too dense").
 * Limits, checked before any device work (GE_ERR_ARG without a GPU): V >= 1; 0 <= row_begin < row_end <= V (0,0 = all rows);
 * rows <= nnz < 2^31; nnz - rows <= rows * (V - 1).  No device: GE_ERR_HIP.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int32_t  vocab_size;          /* V of the whole matrix */
    int32_t  row_begin, row_end;  /* this shard's rows; 0,0 = all */
    int64_t  nnz;                 /* EXACT size of the result, diagonal included */
    uint64_t seed;
    int32_t  device;              /* HIP device ordinal */
    void    *stream;              /* hipStream_t or NULL */
} ge_synth_cfg;
void      ge_synth_cfg_default(ge_synth_cfg *cfg);        /* seed 0xC0FFEE, device 0, everything else 0 */
int32_t   ge_synth_cfg_size(void);
/* The result lives on the device (ge_coo_device); the call returns with the stream drained.  ge_coo_get works on it: its first
 * call for an array copies I, J, X down once and fills row_ptr; *max = (double)0.2f. */
ge_status ge_synth_coo(const ge_synth_cfg *cfg, ge_coo **out);
/* Device views of a result, valid until ge_coo_destroy; all NULL and *device = -1 for a host-resident one (what ge_bca_build
 * returns).  Any out pointer may be NULL. */
ge_status ge_coo_device(const ge_coo *c, int32_t *device, const int32_t **dI, const int32_t **dJ, const float **dX);
/* What the generator did: *draws = t* + 1, the draws up to the one that delivered the last key (a function of the arguments);
 * *kernel_ms = device time of its kernels, sorts and scans (hipEvents); *peak_bytes = the most device memory it held at once,
 * the result included.  GE_ERR_STATE for a ge_coo that was not generated.  Any out pointer may be NULL. */
ge_status ge_coo_synth_stats(const ge_coo *c, int64_t *draws, float *kernel_ms, int64_t *peak_bytes);
/* ge_glove_create on a ge_coo.  cfg->nnz and cfg->xmax are taken from the matrix (each must be 0 or equal to its value),
 * vocab_size must match, the rows must lie inside cfg's row_begin / row_end, a device-resident ge_coo must live on cfg->device.
 * GE_MODE_HOGWILD + GE_SHUFFLE_DEVICE on a device-resident ge_coo: the layout is built from the device arrays in place, no host
 * copy and no upload.  Every other case reads the host arrays (ge_coo_get) and equals ge_glove_create on them.  The handle
 * keeps nothing of the ge_coo: it may be destroyed right after the call. */
ge_status ge_glove_create_coo(const ge_glove_cfg *cfg, const ge_coo *coo, ge_glove **out);

/* ------------------------------------------------------------------------------------------ */
/* Literal-similarity edges.  Replaces the compare loop of Rdf2GrphConverter.convert
 * (J/convert/Rdf2GrphConverter.java:127-186): for one CompareGroup, CompareJob i (J/compare/CompareJob.java:33-51)
 * walks target[startIndex..] and keeps the pairs with metric.similarity(s1, s2) >= threshold; the caller then adds the
 * two directed edges per pair (:163-173).  Methods = Configuration.SimilarityMethod ordinals
 * (J/util/config/Configuration.java:27-29), metrics = SimilarityGroup.toFunction (:201-227). */
enum { GE_SIM_NGRAM_COSINE = 0, GE_SIM_NGRAM_JACCARD = 1, GE_SIM_TOKEN_COSINE = 2, GE_SIM_TOKEN_JACCARD = 3,
       GE_SIM_JAROWINKLER = 4, GE_SIM_LEVENSHTEIN = 5, GE_SIM_NUMERIC = 6,
       GE_SIM_DATE_DAYS = 7, GE_SIM_DATE_MONTHS = 8, GE_SIM_DATE_YEARS = 9 };
enum { GE_TIME_BACKWARDS = 0, GE_TIME_FORWARDS = 1, GE_TIME_BIDIRECTIONAL = 2 };   /* SimilarityGroup.Time (:184-186) */

typedef struct {
    int32_t method;          /* GE_SIM_*                                                                    */
    double  threshold;       /* SimilarityGroup.getThreshold                                                */
    int32_t ngram;           /* getNgram (0 = 3)                                                            */
    double  smooth;          /* getSmooth (0 = 1); Numeric's alpha                                          */
    double  distance;        /* getDistance                                                                 */
    int32_t time;            /* GE_TIME_* (Date* only)                                                      */
    const char *pattern;     /* getPattern: NULL or "iso" = BASIC_ISO_DATE; else the ofPattern subset
                                yyyy|uuuu, MM|M, dd|d, quoted text and literal characters                   */
    int32_t upper_triangle;  /* CompareGroup.upperTriangle: source predicate == target predicate, job i starts
                                at target i+1 (source and target must then be the same list)               */
    int32_t device;          /* HIP device ordinal                                                          */
    int32_t job_begin;       /* multi-GPU sharding: only CompareJobs (source positions) [job_begin, job_end) run;    */
    int32_t job_end;         /*   0,0 = all.  Positions in the result stay global; concatenating the shards' results
                                in job order gives the whole group's result (no collective involved).             */
} ge_sim_cfg;

/* A table of java.lang.String values: string s = UTF-16 code units [offset[s], offset[s+1]) of `units`
 * (what JNI's GetStringChars returns).  At most 1024 units per string that takes part in a comparison. */
typedef struct {
    int32_t         count;
    const int64_t  *offset;  /* count + 1 ascending entries */
    const uint16_t *units;
} ge_strings;

typedef struct ge_sim_pairs ge_sim_pairs;

void ge_sim_cfg_default(ge_sim_cfg *cfg);
int32_t ge_sim_cfg_size(void);      /* sizeof(ge_sim_cfg) as the library was compiled (same purpose as ge_glove_cfg_size) */
/* 1 when Date* can parse with this pattern (NULL/"iso" included), 0 when it is outside the supported subset. */
int32_t ge_sim_pattern_supported(const char *pattern);
/* source[i] / target[j] are positions in `strings` (vertexLabels.getValueAsString of sourceNodes[i] / targetNodes[j]),
 * source_vertex / target_vertex the vertex ids (a job skips its own vertex, CompareJob.java:38).  The result lists
 * (i, j, (float) similarity) in job order -- i ascending, j ascending inside a job -- which is the order results
 * arrive in with `threads: 1`.  A Numeric job that dies in String.substring (Numeric.java:36) yields nothing, as its
 * ExecutionException does in the reference (Rdf2GrphConverter.java:176-178).  A job dies when one of the targets it
 * reaches -- at or after its start, on another vertex than its own -- is non-empty and shorter than the '^' position of
 * the job's label; a short target on the job's own vertex is skipped before the substring and kills nothing. */
ge_status ge_similarity_pairs(const ge_strings *strings,
                              const int32_t *source, const int32_t *source_vertex, int32_t n_source,
                              const int32_t *target, const int32_t *target_vertex, int32_t n_target,
                              const ge_sim_cfg *cfg, ge_sim_pairs **result);
/* Host views, valid until ge_sim_pairs_destroy.  Any out pointer may be NULL. */
ge_status ge_sim_pairs_get(const ge_sim_pairs *r, int64_t *count, const int32_t **source_pos, const int32_t **target_pos,
                           const float **similarity);
void ge_sim_pairs_destroy(ge_sim_pairs *r);

/* ------------------------------------------------------------------------------------------ */
/* ------------------------------------------------------------------------------------------ */
/* Where the context rows of a handle live on the device (ge_sync works on these; tests and tools wrap them zero-copy).  dtype GE_DTYPE_F32:
 * `table` is float[vocab_size*row_stride] and the hub fields are NULL/0.  GE_DTYPE_BF16: `table` is bf16[vocab_size*dim];
 * a column v with hub_index[v] >= 0 keeps its current value in hub_rows[hub_index[v]*dim ..] (fp32 master row; the
 * bf16 copy of such a row is stale until extraction).  Which columns are hubs is decided per handle from ITS nonzeros. */
typedef struct {
    void          *table;
    int32_t        dtype;        /* GE_DTYPE_* */
    float         *hub_rows;     /* [n_hub x dim] */
    const int32_t *hub_index;    /* [vocab_size], device memory */
    int32_t        n_hub, vocab_size, dim;
    int32_t        row_stride;   /* elements of `table`'s dtype between consecutive rows of `table`.  fp32 GE_MODE_HOGWILD handles keep
                                    FAT rows (a row's bias at [dim]; width dim + 4, widened to whole 64-byte lines where that costs under
                                    10 %: dim 200 -> 208 floats) inside records [row | accumulator row] that start on 64-byte boundaries:
                                    row_stride = the record, 2 row widths rounded up to 16 floats (dim 200: 416; ge_glove_info.row_stride
                                    says what a handle uses); bf16 rows lead records [bf16 row padded to 16 B | fp32 accumulator row, fat:
                                    gradSq (dim) | its bias accumulator | the bias | 2 x 0]: row_stride = that record in bf16
                                    elements; GE_LAYOUT_SEPARATE_TABLES: the row width itself */
    float         *accum;        /* gradSqContext (Adam/AMSGrad: M1context); fp32 always; fat like `table` when that is fp32 */
    int32_t        accum_stride; /* floats between consecutive rows of `accum` (its bias accumulator at [dim] when fat)             */
    float         *bias;         /* cBias[v] = bias[v * bias_stride]: a vector of its own (stride 1), column [dim] of the fat fp32 row,
                                    or -- bf16 rows, which cannot carry it -- column [dim + 1] of the accumulator row                */
    int32_t        bias_stride;
    float         *accum_bias;   /* gradSqCBias[v] = accum_bias[v * accum_bias_stride] (fat: column [dim] of the accumulator row)      */
    int32_t        accum_bias_stride;
} ge_context_layout;
ge_status ge_glove_context_layout(ge_glove *h, ge_context_layout *out);

/* The elementwise half of one exchange step for a GE_DTYPE_BF16 context table (what ge_sync runs for bf16 rows; exported for
 * its parity test).  One pass over device memory on `stream`, asynchronous:
 *   land != 0:  row value += wire - own, base += wire - own   (`wire` = the all-reduced sum of every rank's bf16 delta, `own`
 *               this rank's part of it: the difference is what the others sent);
 *   take != 0:  d = bf16(row value - base) (before landing); own = d; base += d.  `wire` is never written here: it is the
 *               receive buffer of the all-reduce that follows (send buffer own).
 * A row's value lives in hub_rows[hub_index[v]] (fp32 master) when the column is a hub on this rank, else in the bf16 table.
 * The table's rows are `row_stride` bf16 elements apart (a multiple of 4; ge_context_layout.row_stride).
 * `base` is float[vocab_size*dim] for EVERY row (start: the row values widened), wire / own are bf16[vocab_size*dim].  Landed
 * ordinary rows are re-narrowed with stochastic rounding drawn from `seed` (a new one every turn); that rounding is part of
 * value - base and is fed back with the next delta. */
ge_status ge_exchange_turn_bf16(uint16_t *table, int32_t row_stride, float *hub_rows, const int32_t *hub_index, int32_t vocab_size, int32_t dim,
                                float *base, uint16_t *wire, uint16_t *own, int32_t land, int32_t take, uint32_t seed, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* Multi-GPU trainer behind the C ABI (north_star: "rows shard across the 8 GPUs of one node with a periodic
 * RCCL all-reduce of the context factors").  One ge_glove handle per GPU (cfg.device, cfg.row_begin/row_end = its block of
 * focus rows, its nonzeros), one ge_sync per handle; the host runs the handles in lockstep -- one process per GPU, or one
 * thread per GPU inside one process (the JVM) -- and after every ge_glove_epoch calls ge_sync_turn (or ge_sync_sync).
 * The reference is a single JVM and has no counterpart; the merge rule is product semantics and lives in the library:
 *   context rows and both AdaGrad accumulators: the ranks' deltas ADD; cBias: the MEAN over the ranks that moved the element
 *   (the reference updates biases without a learning rate, J/opt/grad/Adagrad.java:88-89); the accumulators are reconciled
 *   only every accum_every-th exchange.  GE_MODE_HOGWILD + GE_OPT_ADAGRAD handles (fp32 or bf16 rows). */
typedef struct ge_sync ge_sync;
typedef struct ge_local_group ge_local_group;

/* A collective supplied by the host instead of RCCL (tests: torch.distributed / gloo with two ranks on one GPU; the C++ CLI:
 * N ranks inside one process).  buf is DEVICE memory of `count` elements of GE_DTYPE_F32 or GE_DTYPE_BF16; the library has
 * drained its stream before it calls.  start: begin summing buf over all ranks in place, *ticket identifies the operation;
 * wait: return when that sum is in buf; broadcast: every rank's buf becomes rank src's (blocking).  Return GE_OK or GE_ERR_*. */
typedef struct {
    void *user;
    ge_status (*start)(void *user, void *buf, int64_t count, int32_t dtype, void **ticket);
    ge_status (*wait)(void *user, void *ticket);
    ge_status (*broadcast)(void *user, void *buf, int64_t count, int32_t dtype, int32_t src);
} ge_transport;

typedef struct {
    int32_t world, rank;           /* ranks = GPUs; world == 1: every call is a no-op                                        */
    int32_t wire;                  /* GE_DTYPE_BF16: the deltas of the row / accumulator tables travel as bf16 (half the bytes
                                      over xGMI; what the rounding drops is fed back with the next delta); GE_DTYPE_F32        */
    int32_t accum_every;           /* accumulators every Nth exchange (0 = 4)                                                  */
    const ge_transport *transport; /* NULL: RCCL (the library opens librccl.so.1 at run time) ...                              */
    const void *rccl_id;           /* ... with this 128-byte ncclUniqueId: ge_rccl_unique_id on rank 0, handed to every rank   */
    ge_local_group *local_group;   /* or: the ranks are threads of THIS process and meet in host memory (any number of devices;
                                      a rehearsal of an N-rank run on fewer GPUs, blocking, no overlap)                        */
} ge_sync_cfg;

/* The ranks of one process (one host thread per rank): created once, handed to every rank's ge_sync_cfg, destroyed after the
 * last ge_sync_destroy. */
ge_status ge_local_group_create(int32_t world, ge_local_group **out);
void ge_local_group_destroy(ge_local_group *g);
/* A rank thread that fails OUTSIDE the ge_sync calls (its ge_glove_create, its epoch) calls this before it leaves: every peer
 * waiting in -- or arriving at -- an exchange of the group returns GE_ERR_STATE instead of waiting for a rank that will not
 * come.  (A rank that fails INSIDE a ge_sync call aborts its group itself.)  The group stays aborted. */
void ge_local_group_abort(ge_local_group *g);

ge_status ge_rccl_unique_id(void *id128);
/* Opens RCCL, makes a one-rank communicator on `device`, runs a sum and a broadcast through it and checks the data: what a
 * single-GPU machine can verify of the RCCL path. */
ge_status ge_rccl_selftest(int32_t device);
int32_t ge_sync_cfg_size(void);
/* Collective: every rank calls it (RCCL: ncclCommInitRank inside).  The base of every table is its value NOW.  A ge_sync
 * works on its handle's device tables: destroy it before the ge_glove it was created for. */
ge_status ge_sync_create(ge_glove *h, const ge_sync_cfg *cfg, ge_sync **out);
/* begin = take: the deltas since the last take go on the wire (everything != 0: accumulators too), asynchronously on RCCL's
 * own stream.  finish = land: waits for them and adds what the OTHER ranks sent.  turn = finish, then begin: the all-reduce of
 * step k runs under ge_glove_epoch of step k+1 (launch that epoch with cfg.workers = -256 so RCCL's kernels find room), and a
 * rank sees the others' moves one step late.  sync = turn, then finish: exact replicas after every step, nothing left in flight.  All enqueue on the
 * handle's stream and return; none blocks the host with RCCL. */
ge_status ge_sync_begin(ge_sync *s, int32_t everything);
ge_status ge_sync_finish(ge_sync *s);
ge_status ge_sync_turn(ge_sync *s);
ge_status ge_sync_sync(ge_sync *s);
/* One epoch of a sharded run, to be called INSTEAD of ge_glove_epoch by every rank (collective).  On the way the HUB rows of the
 * context side -- the union of the ranks' busy columns (count on a rank >= max(256, N_rank / 20 480); from four ranks on the divisor grows with the ranks), a few thousand rows -- are
 * reconciled `segments` times in small fp32 all-reduces (<= 0: as often as the busiest column asks for -- one exchange per 65 536
 * updates that all ranks together put on it, at least max(8, ranks) --; at most 128 live, 64 in segments).
 * Without it eight ranks that each push a busy row for a whole epoch from the same start overshoot where one GPU settles, and with too few
 * exchanges for a very busy column the run leaves the single-GPU trajectory (measured: DESIGN.md 7); inside a GPU the same rows are held
 * together by publishing deltas every few updates, across GPUs by this.  Two forms:
 *   live      (over RCCL or a local group): the epoch is ONE launch and the exchanges run BESIDE it on a stream of their own --
 *             the epoch kernel moves its hub columns by atomic adds only (a sharded handle counts every column that is busy on the rank
 *             among them), so the other ranks' deltas are added the same way (k_live_take / k_live_land) -- paced by the epoch's
 *             ticket counter; the epoch kernel never waits.  Should the exchanges fall behind the epoch (a quarter of them a whole
 *             interval late on half of the ranks, two epochs running: a slow transport, epochs of a few milliseconds), the ranks agree to
 *             continue in segments.
 *             bf16 rows: on the fp32 master rows of the columns that are hubs on every rank (the few at the threshold that are not wait for
 *             the end of the epoch).
 *   segments  (a host transport, GE_SYNC_EPOCH=segments, a run that fell behind): the epoch runs in `segments` launches and behind each one the hub
 *             rows are reconciled exactly (both accumulators summed, cBias averaged over the ranks that moved it, the parameter rows' summed
 *             deltas scaled per element by sqrt((G0 + E / W) / (G0 + E)) -- G0 the accumulator at the last exchange, E this exchange's summed
 *             accumulator deltas: every rank stepped without the others' gradients in its accumulator, and W such pushes summed as they
 *             are overshoot by up to sqrt(W); GE_SYNC_MERGE=sum turns the scaling off --; the live form merges the same way).
 * Both end the epoch with that exact exchange of all hub rows.  ge_sync_turn / ge_sync_sync follow as before (they find nothing left to
 * do for the hub rows).  *cost_sum as ge_glove_epoch.  A bf16 handle reads and writes a hub row where IT keeps it: the fp32 master row
 * of a column that is a hub on this rank, else the bf16 table entry, stochastically rounded.  A one-rank run and a run without hub
 * columns get one plain ge_glove_epoch. */
ge_status ge_sync_epoch(ge_sync *s, int32_t iteration, int32_t segments, double *cost_sum);
/* The hub rows of this run (*count of them, ascending; out may be NULL or shorter), and ONE small exchange of them now (collective; what
 * ge_sync_epoch does behind every segment) -- for a host that cuts its epochs itself. */
ge_status ge_sync_hub_rows(ge_sync *s, int32_t *out, int32_t capacity, int32_t *count);
ge_status ge_sync_hub_exchange(ge_sync *s);
/* One LIVE exchange now (collective; GE_ERR_STATE when the run has no live rows), and what ge_sync_epoch(s, ., segments, .) will do:
 * *live = 1 beside the running kernel / 0 in segments, *exchanges per epoch, *live_rows = rows exchanged live (0 in segments). */
ge_status ge_sync_hub_exchange_live(ge_sync *s);
ge_status ge_sync_live_rows(ge_sync *s, int32_t *out, int32_t capacity, int32_t *count);      /* the rows a live exchange covers (ascending; as ge_sync_hub_rows) */
ge_status ge_sync_hub_plan(ge_sync *s, int32_t segments, int32_t *live, int32_t *exchanges, int32_t *live_rows);
/* Ends a run: lands what is in flight, exchanges everything not sent yet, then every rank takes rank src's fp32 tables. */
ge_status ge_sync_replicate(ge_sync *s, int32_t src);
/* n host doubles summed (op 0) or maximised (op 1) over the ranks through RCCL: the epoch's cost (Optimizer.java:94-96 needs
 * the sum over all jobs), BookmarkColoring's max over shards.  Blocking, and ordered on the communicator BEHIND whatever
 * ge_sync_turn has put on the wire: reduce an epoch's cost BEFORE that epoch's ge_sync_turn (epoch -> allreduce(cost) ->
 * turn), or the host waits for the whole context all-reduce and the overlap with the next epoch is lost. */
ge_status ge_sync_allreduce_f64(ge_sync *s, double *values, int32_t n, int32_t op);
void ge_sync_destroy(ge_sync *s);

/* ------------------------------------------------------------------------------------------
 * PCA of the trained vectors (the `pca: { variance }` block of the shipped YAMLs).  The reference parses that block and
 * prints it (J/Main.java:43-44) but never reduces anything, so these are product semantics:
 *   moments   mean[d] = sum_r x[r][d] / n,  cov[a][b] = sum_r (x[r][a] - mean[a]) (x[r][b] - mean[b]) / (n - 1), accumulated
 *             in fp64 on the device (k_pca_gram, fp64 matrix cores); a fixed partition of the rows and a fixed-order
 *             reduction, no floating-point atomics: the same input on the same device gives the same bytes, call after call.
 *             Non-finite moments are GE_ERR_ARG ("non-finite input").
 *   model     eigen-decomposition of cov on the host in fp64 (Householder tridiagonalisation + implicit QL, own code).
 *             Eigenvalues descending, negative rounding residue clamped to 0; in every component the entry of largest
 *             magnitude is positive (lowest index on a tie).
 *   k         the smallest k >= 1 with  sum_{c<k} lambda_c >= variance * sum_c lambda_c  (fp64, in that order), then capped
 *             by max_components.  Constant input (sum lambda = 0): k = 1 and a projection of zeros.
 *   transform out[r][c] = sum_d (x[r][d] - mean[d]) * components[d][c]: centred first (in fp64, rounded to fp32 once), then
 *             the products in fp32 in ascending d (k_pca_project, an fmaf chain on the fp32 matrix cores).
 * Limits: 2 <= n_rows, 1 <= dim <= 1024, variance in (0, 1], max_components >= 0; anything else is GE_ERR_ARG, checked
 * before any device work.  No device: GE_ERR_HIP.
 * ---------------------------------------------------------------------------------------- */
typedef struct ge_pca ge_pca;
typedef struct {
    double  variance;        /* pca.variance: keep the fewest leading components whose eigenvalues sum to >= variance * total */
    int32_t max_components;  /* > 0: never keep more than this many; 0 = no cap */
    int32_t device;          /* HIP device ordinal */
    void   *stream;          /* hipStream_t or NULL */
} ge_pca_cfg;
void      ge_pca_cfg_default(ge_pca_cfg *cfg);            /* variance 0.95, no cap, device 0 */
int32_t   ge_pca_cfg_size(void);

/* rows: HOST float[n_rows * dim], row-major; uploaded in slabs (no second copy of the table on either side). */
ge_status ge_pca_fit(const float *rows, int64_t n_rows, int32_t dim, const ge_pca_cfg *cfg, ge_pca **out);
/* The same on the vectors a trainer handle holds -- (focus + context) / 2, what ge_glove_extract_f32 returns -- without the
 * trip through host memory; bit for bit the model ge_pca_fit builds from that output.  Runs on the handle's device. */
ge_status ge_glove_pca_fit(ge_glove *h, const ge_pca_cfg *cfg, ge_pca **out);
/* HOST ONLY, needs no device: the model from moments a caller already has (a sharded run sums its shards' moments).
 * mean[dim], cov[dim*dim] symmetric, the covariance with divisor n_rows - 1. */
ge_status ge_pca_from_moments(const double *mean, const double *cov, int32_t dim, int64_t n_rows,
                              const ge_pca_cfg *cfg, ge_pca **out);
/* Host views, valid until ge_pca_destroy; any out pointer may be NULL.  components: double[dim*dim], column c (element
 * [d*dim + c]) is the unit eigenvector of the c-th LARGEST eigenvalue; eigenvalues: double[dim] descending; *k = kept. */
ge_status ge_pca_get(const ge_pca *p, int32_t *dim, int32_t *k, int64_t *n_rows, const double **mean, const double **cov,
                     const double **eigenvalues, const double **components);
/* out: HOST float[n_rows * k] */
ge_status ge_pca_transform(const ge_pca *p, const float *rows, int64_t n_rows, float *out);
ge_status ge_glove_pca_transform(const ge_pca *p, ge_glove *h, float *out);     /* out: HOST float[V * k] */
/* Device time of the handle's last moment pass (ge_pca_fit, ge_glove_pca_fit) and last projection, hipEvents around the
 * kernels, in milliseconds (0 = none ran); uploads are not counted.  Either out pointer may be NULL. */
ge_status ge_pca_last_kernel_ms(const ge_pca *p, float *fit_ms, float *transform_ms);
void      ge_pca_destroy(ge_pca *p);

/* ------------------------------------------------------------------------------------------
 * Top-k nearest neighbours over a table of vectors: which rows lie closest to this one?  Exact (every candidate is scored),
 * on one device.  The reference stops at the vectors file and has no counterpart, so these are product semantics:
 *   prepared row  COSINE: n = sqrt(sum_d x_d^2), accumulated in fp64 in ascending d; xh_d = (float)((double)x_d / n), rounded
 *                 once; a zero row stays zero.  DOT: xh = x.  Query vectors given as values are prepared the same way.
 *   score         s(q, c) = sum_d xh_q[d] * xh_c[d], an fp32 fmaf chain from 0 in ascending d (k_nn_score_select on the fp32
 *                 matrix cores, which give exactly that chain).  A score depends on its two rows only: not on the tile, the
 *                 batch or the other candidates.  A sum that overflows to NaN ranks, and is reported, as -inf.
 *   result        per query the first k candidates in a total order: score descending as fp32 compares them (so -0 = +0), equal
 *                 scores by ascending row id.  With exclude_self the query's own row id is not a candidate.  out_index holds
 *                 ORIGINAL row ids.  Scores are deterministic and the order is total, so the bytes of a result are a function
 *                 of the input alone: no float atomics, no order-dependent selection.
 * Limits, checked before any device work (GE_ERR_ARG without a GPU): 1 <= dim <= 1024; 1 <= k <= 128;
 * k <= candidates - (exclude_self ? 1 : 0); 1 <= n_rows < 2^31 - 1 and n_rows * dim <= 2^35 floats (what one device allocation
 * of the index may hold); the subset strictly ascending and in range; query ids that are members of the index; a known metric.
 * Non-finite input rows or query vectors: GE_ERR_ARG ("non-finite input").  No device: GE_ERR_HIP.
 * ---------------------------------------------------------------------------------------- */
typedef struct ge_nn ge_nn;
enum { GE_NN_COSINE = 0, GE_NN_DOT = 1 };
typedef struct {
    int32_t metric;          /* GE_NN_COSINE or GE_NN_DOT */
    int32_t device;          /* HIP device ordinal */
    void   *stream;          /* hipStream_t or NULL */
} ge_nn_cfg;
void      ge_nn_cfg_default(ge_nn_cfg *cfg);              /* cosine, device 0, null stream */
int32_t   ge_nn_cfg_size(void);
/* rows: HOST float[n_rows * dim], row-major; uploaded in slabs.  subset: NULL (all rows are candidates; n_subset is ignored)
 * or n_subset strictly ascending row ids = the candidates.  The index lives on the device until ge_nn_destroy. */
ge_status ge_nn_create(const float *rows, int64_t n_rows, int32_t dim, const int32_t *subset, int64_t n_subset,
                       const ge_nn_cfg *cfg, ge_nn **out);
/* The same on the vectors a trainer handle holds -- (focus + context) / 2, what ge_glove_extract_f32 returns -- without the
 * trip through host memory; bit for bit the index, and hence the results, ge_nn_create builds from that output.  Runs on the
 * handle's device and writes no trainer table. */
ge_status ge_glove_nn_create(ge_glove *h, const int32_t *subset, int64_t n_subset, const ge_nn_cfg *cfg, ge_nn **out);
/* query_ids: NULL (every indexed row, in order; n_queries must then be the number of indexed rows) or n_queries row ids that
 * are members of the index.  out_index, out_score: HOST [n_queries * k] each. */
ge_status ge_nn_query_rows(ge_nn *p, const int32_t *query_ids, int64_t n_queries, int32_t k, int32_t exclude_self,
                           int32_t *out_index, float *out_score);
/* vectors: HOST float[n_queries * dim] */
ge_status ge_nn_query_vectors(ge_nn *p, const float *vectors, int64_t n_queries, int32_t k,
                              int32_t *out_index, float *out_score);
ge_status ge_nn_get(const ge_nn *p, int64_t *n_indexed, int32_t *dim, int32_t *metric);   /* any out pointer may be NULL */
/* Device time of building the index and of the handle's last query call (its kernels, query preparation included), hipEvents
 * around the kernels, in milliseconds (0 = none ran); copies are not counted.  Either out pointer may be NULL. */
ge_status ge_nn_last_kernel_ms(const ge_nn *p, float *prepare_ms, float *query_ms);
void      ge_nn_destroy(ge_nn *p);

/* ------------------------------------------------------------------------------------------
 * Held-out evaluation: how well do the vectors predict co-occurrences the trainer never saw?  The cost term of
 * Adagrad.createJob (J/opt/grad/Adagrad.java:60-75), computed and not applied, for a set of nonzeros (I[k], J[k], X[k]),
 * k = 0 .. n-1, that need not be the handle's own: arbitrary pairs, read from whichever layout the handle keeps its tables in
 * (plain tables, records, packed records, bf16 rows with fp32 hub masters, a shard).  The arithmetic is the bit-exact
 * trainer's (csrc/ge_exact.h exact_update), stopped before the update:
 *   s          the fp32 sum over ascending d of the fp32 products focus[i][d] * context[j][d]; products not fused, sum from 0.0f.
 *   l, w       cost_terms<true> (csrc/ge_cost.h) with the handle's cost kind and the handle's xmax.
 *   residual   ic = (float)((double)s + ((double)(fBias[i] + cBias[j]) - l));  wc = w * ic.
 *   term       t_k = (0.5 * (double)wc) * (double)ic, an fp64 value: what the exact kernel adds to its job accumulator.
 *   cost_sum   fp64, over a fixed partition: S_b = the sum of t_k over k in [1024 b, 1024 (b + 1)) in ascending k, from 0.0;
 *              cost_sum = the sum of S_b in ascending b, from 0.0.  No floating-point atomics: the same input gives the same
 *              bytes on every run and every machine.
 *   bf16       a row is read where the handle keeps it: the fp32 master row when hub_index[j] >= 0, else the bf16 entry widened
 *              exactly; from there the same arithmetic.
 *   pure read  no table is written; neither the RNG state nor the permutation is touched.
 * Limits, checked on the host before any device work (GE_ERR_ARG): 1 <= n < 2^31; I[k] inside the handle's owned rows
 * [row_begin, row_end); J[k] in [0, V); X[k] finite and > 0, and < 1 for pGloVe; no null argument.
 * The set is a handle of its own (evaluated after every epoch, uploaded once).  Creation may reorder the set by focus row so
 * that consecutive nonzeros share rows; results always come back in the caller's k order and cost_sum follows the partition
 * above in the caller's k.  ge_glove_eval_run runs on the trainer handle's stream and is blocking, like every call on a handle.
 * ---------------------------------------------------------------------------------------- */
typedef struct ge_eval ge_eval;
ge_status ge_glove_eval_create(ge_glove *h, const int32_t *I, const int32_t *J, const float *X, int64_t n, ge_eval **out);
/* out_residual: HOST float[n] or NULL; out_term: HOST double[n] or NULL; both in the caller's k order.  cost_sum may be NULL. */
ge_status ge_glove_eval_run(ge_eval *e, float *out_residual, double *out_term, double *cost_sum);
/* Device time of the last run's kernels (hipEvents around them; copies not counted), in milliseconds; 0 = none ran. */
ge_status ge_eval_last_kernel_ms(const ge_eval *e, float *ms);
/* *n = nonzeros of the set; *reordered = 1 when creation sorted it by focus row (0: it arrived so).  Either may be NULL. */
ge_status ge_eval_get(const ge_eval *e, int64_t *n, int32_t *reordered);
void      ge_eval_destroy(ge_eval *e);     /* before the ge_glove it was created for */
/* The split rule, HOST ONLY (no device): mask[k] = 1 when nonzero k is held out, i.e. when
 * hi(SM(seed ^ 0x484F4C444F5554, k)) < T, T = floor(fraction * 2^32) computed in fp64 (SM, hi: the notation of the synthetic
 * matrix above).  A function of (seed, k, fraction) alone.  fraction outside (0, 0.5] (NaN included): GE_ERR_ARG. */
ge_status ge_holdout_mask(uint64_t seed, int64_t n, double fraction, uint8_t *mask);
/* The late-vertex rule of the CLI's fold-in split (see "Fold-in"), HOST ONLY: mask[v] = 1 when vertex v is late, i.e. when
 * hi(SM(seed ^ 0x464F4C44494E, v)) < T, T = floor(fraction * 2^32) computed in fp64.  A function of (seed, v, fraction) alone.
 * fraction outside (0, 0.5] (NaN included): GE_ERR_ARG. */
ge_status ge_foldin_mask(uint64_t seed, int64_t n, double fraction, uint8_t *mask);

/* ------------------------------------------------------------------------------------------
 * Ranking: at which place does column J[k] stand among all V columns when they are ordered by the model's own prediction for
 * row I[k]?  Its summaries, MRR and hits@k, are the usual measures of a graph embedding.  The reference has no counterpart, so
 * these are product semantics.  A rank set is n pairs (I[k], J[k]), k = 0 .. n-1, each with an optional filter list F_k (the
 * known positives of the row, which a "filtered" rank leaves out): filter_ptr[n + 1] (ascending offsets) into filter_idx, the
 * ids of a list in [0, V) and strictly ascending; filter_ptr == NULL: no filter.
 *   score      a = focus[I[k]], b = context[c], D = dim:  s(k, c) is the fp32 fmaf chain from 0.0f over ascending d,
 *              s = fmaf(a[d], b[d], s);  z(k, c) = s(k, c) + cBias[c], one fp32 add.  A NaN z ranks, and is reported, as -inf.
 *              fBias[i] is the same for every candidate of a query and is not part of z.  Rows are read where the handle
 *              keeps them, by the rules of ge_glove_eval_*: plain tables, records, packed records, a shard's rebased focus
 *              rows, bf16 rows widened exactly and the fp32 master row when hub_index[c] >= 0.  A score depends on its two
 *              rows and the bias only: not on the tile, the batch or the other pairs.
 *   rank       candidate c precedes j when z(k, c) > z(k, j) as fp32 compares, or z(k, c) == z(k, j) and c < j: the total
 *              order of ge_nn_* (so -0 = +0).   rank[k] = 1 + #{ c in [0, V), c != J[k], c not in F_k : c precedes J[k] }.
 *              J[k] inside its own list is ignored.  Ranks are integers and the order is total, so the bytes of a result are
 *              a function of the input alone; counts are combined by integer atomics, there are no floating-point atomics.
 *   summary    computed on the host from the ranks: n; mrr = (the fp64 sum of 1.0 / rank[k] in ascending k, from 0.0) / n;
 *              mean_rank in fp64, the same way; hits1, hits10, hits100 = how many ranks are <= 1, <= 10, <= 100.
 *   pure read  no trainer table is written; neither the RNG state nor the permutation is touched.
 * Limits, checked on the host before any device work (GE_ERR_ARG): 1 <= n < 2^31; 1 <= dim <= 1024; I[k] inside the handle's
 * owned rows [row_begin, row_end); J[k] and every filter id in [0, V); lists strictly ascending; filter_ptr[0] == 0 and
 * filter_ptr non-decreasing; fewer than 2^35 filter entries in all; no null mandatory argument.  (What needs no handle -- the
 * null arguments, n, the shape and order of the lists, ids below 0 -- is refused first, so without a device as well.)
 * Every handle mode is supported.  The set and its lists are uploaded once at creation; ge_glove_rank_run may be called after
 * any epoch, runs on the trainer handle's stream and is blocking.
 * Device memory: the tables are NOT read in place.  Every run stages the n query focus rows and the whole context table into
 * dense fp32 buffers of row length D4 = dim rounded up to 4 (one read and one write of the context table; the tables move
 * between epochs), so a set holds (V + n) * D4 * 4 bytes + 4 V (biases) + 16 n + 8 per filter entry until ge_rank_destroy.
 * ---------------------------------------------------------------------------------------- */
typedef struct ge_rank ge_rank;
typedef struct { int64_t n; double mrr, mean_rank; int64_t hits1, hits10, hits100; } ge_rank_summary;
ge_status ge_glove_rank_create(ge_glove *h, const int32_t *I, const int32_t *J, int64_t n,
                               const int64_t *filter_ptr, const int32_t *filter_idx, ge_rank **out);
/* out_rank: HOST int32[n] or NULL; out_score: HOST float[n] (z of the target) or NULL; both in the caller's k order.  summary may be NULL. */
ge_status ge_glove_rank_run(ge_rank *r, int32_t *out_rank, float *out_score, ge_rank_summary *summary);
/* Device time of the last run's kernels (hipEvents around them; copies not counted), in milliseconds; 0 = none ran. */
ge_status ge_rank_last_kernel_ms(const ge_rank *r, float *ms);
/* The same split into staging, the target and filter scores, and the dense count; any out pointer may be NULL. */
ge_status ge_rank_last_phase_ms(const ge_rank *r, float *stage_ms, float *gather_ms, float *count_ms);
/* *n = pairs; *candidates = V; *dim; *ranges = the candidate ranges the last run's grid had (0 before the first run: the
 * results do not depend on it).  Any out pointer may be NULL. */
ge_status ge_rank_get(const ge_rank *r, int64_t *n, int64_t *candidates, int32_t *dim, int32_t *ranges);
int32_t   ge_rank_summary_size(void);
void      ge_rank_destroy(ge_rank *r);     /* before the ge_glove it was created for */

/* ------------------------------------------------------------------------------------------
 * Prediction: which columns does the model expect in row I[k]?  The columns at places 1, 2, .., K of the order that
 * ge_glove_rank_* measures places in -- the missing links of a trained graph embedding.  The reference has no counterpart, so
 * these are product semantics.  A prediction set is n query rows I[k], k = 0 .. n-1 (rows may repeat), with three optional parts:
 *   filter     lists F_k exactly as for ge_glove_rank_create: filter_ptr[n + 1] (ascending offsets) into filter_idx, the ids of
 *              a list in [0, V) and strictly ascending; filter_ptr == NULL: no filter.
 *   subset     a candidate set S shared by all queries: n_subset strictly ascending ids in [0, V), as the subset of
 *              ge_nn_create; NULL: all V columns (n_subset is ignored).
 *   exclude_self   non-zero: column I[k] is not a candidate of query k.
 *   score      z(k, c) is the z of the Ranking section: the fp32 fmaf chain from 0.0f over ascending d of
 *              focus[I[k]][d] * context[c][d], plus cBias[c] in one fp32 add; a NaN z counts, and is reported, as -inf; fBias is
 *              left out.  Rows are read where the handle keeps them, by the rules of ge_glove_eval_*: every mode, records,
 *              packed records, a shard's rebased focus rows, bf16 rows widened exactly and the fp32 master row when
 *              hub_index[c] >= 0.  A score depends on its two rows and the bias only: not on the tile, the grid or the batch.
 *   candidates C_k = S \ F_k \ ({I[k]} if exclude_self), ordered by the total order of ge_nn_*: z descending as fp32 compares
 *              (so -0 = +0), equal z by ascending column id.  A filter id outside S is legal and ignored; an empty C_k is legal.
 *   result     for a run with 1 <= K <= 128: out_count[k] = min(K, |C_k|); out_index[k * K + t], out_score[k * K + t] = the
 *              t-th candidate of that order and its z, t < out_count[k]; the remaining slots hold (-1, -inf).  A real
 *              candidate whose z is -inf comes before the fill.  So ge_glove_rank_run on the pair (I[k], out_index[k * K + t])
 *              with the list F_k (plus I[k] under exclude_self; S = all columns) returns rank t + 1 and the same score bits.
 *   bytes      a function of the input alone: no floating-point atomics, no order-dependent selection.
 *   pure read  no trainer table is written; neither the RNG state nor the permutation is touched.
 * Limits, checked on the host before any device work (GE_ERR_ARG): 1 <= n < 2^31; 1 <= dim <= 1024; I[k] inside the handle's
 * owned rows [row_begin, row_end); every filter id in [0, V); lists strictly ascending; filter_ptr[0] == 0 and filter_ptr
 * non-decreasing; fewer than 2^35 filter entries in all; the subset strictly ascending, in [0, V) and n_subset >= 1;
 * 1 <= K <= 128; no null mandatory argument.  (What needs no handle -- the null arguments, n, the shape and order of the lists
 * and of the subset, ids below 0, K -- is refused first, so without a device as well.)
 * Every handle mode is supported.  The set is uploaded once at creation (filter lists translated to candidate positions);
 * ge_glove_predict_run may be called after any epoch and re-stages each time, runs on the trainer handle's stream and is blocking.
 * Device memory: the tables are NOT read in place.  Every run stages the n query focus rows and the |S| candidate context rows
 * into dense fp32 buffers of row length D4 = dim rounded up to 4, so a set holds (|S| + n) * D4 * 4 bytes + 4 |S| (biases) +
 * 4 |S| (the subset, when given) + 16 n + 4 per filter entry inside S until ge_predict_destroy.  A run holds, while it lasts,
 * the partial lists of its candidate ranges (8 K bytes per query and range, at most 128 MB: more queries go in batches, each
 * sized by the range count of its own grid) and 8 K + 4 bytes of results per query of a batch.
 * ---------------------------------------------------------------------------------------- */
typedef struct ge_predict ge_predict;
ge_status ge_glove_predict_create(ge_glove *h, const int32_t *I, int64_t n,
                                  const int64_t *filter_ptr, const int32_t *filter_idx,
                                  const int32_t *subset, int64_t n_subset, int32_t exclude_self, ge_predict **out);
/* out_index: HOST int32[n * K], out_score: HOST float[n * K], out_count: HOST int32[n]; each may be NULL. */
ge_status ge_glove_predict_run(ge_predict *p, int32_t K, int32_t *out_index, float *out_score, int32_t *out_count);
/* Device time of the last run's kernels, split into staging, score-and-select and the merge (hipEvents around them; copies
 * not counted), in milliseconds; 0 = none ran.  Any out pointer may be NULL. */
ge_status ge_predict_last_kernel_ms(const ge_predict *p, float *stage_ms, float *select_ms, float *merge_ms);
/* *n = query rows; *candidates = |S|; *dim; *ranges = the candidate ranges the last run's grid had (0 before the first run: the
 * results do not depend on it).  Any out pointer may be NULL. */
ge_status ge_predict_get(const ge_predict *p, int64_t *n, int64_t *candidates, int32_t *dim, int32_t *ranges);
void      ge_predict_destroy(ge_predict *p);   /* before the ge_glove it was created for */

/* ------------------------------------------------------------------------------------------
 * Clustering: which vertices belong together?  Lloyd's k-means over a table of vectors, on one device.  The reference stops at
 * the vectors file and has no counterpart, so these are product semantics:
 *   indexed rows  as the nearest-neighbour index: host rows with an optional strictly ascending subset, or the vectors of a
 *                 trainer handle.  Position p = 0 .. n-1 is the p-th indexed row; labels are centroid ids 0 .. K-1 and every
 *                 per-row result is indexed by position.
 *   metric        GE_KM_COSINE (spherical k-means): a row is prepared as GE_NN_COSINE prepares it -- n = sqrt(sum_d x_d^2)
 *                 accumulated in fp64 in ascending d, xh_d = (float)((double)x_d / n), a zero row stays zero.
 *                 GE_KM_EUCLID: xh = x.
 *   score         s(p, c) is the fp32 fmaf chain from 0.0f over ascending d, s = fmaf(xh_p[d], cen_c[d], s) (k_km_assign on the
 *                 fp32 matrix cores, which give exactly that chain);  z(p, c) = s(p, c) + h_c, one fp32 add.  COSINE: h_c = 0.0f.
 *                 EUCLID: h_c = (float)(-0.5 * q_c), q_c = the fp64 sum from 0.0 over ascending d of the unfused products
 *                 (double)cen_c[d] * (double)cen_c[d]: argmax_c z = argmin_c |x - cen_c|^2.  A NaN z counts as -inf.
 *   assign        label[p] = the c that comes first in the total order of the nearest-neighbour results: z descending as fp32
 *                 compares (so -0 = +0), equal z by ascending c.  best[p] = z(p, label[p]).  A label depends on its row and the
 *                 centroids only: not on the tile, the batch or the order in which anything arrives.
 *   update        the members of c are the positions with label == c in ascending p, n_c their number.  S_c[d] is an fp64 sum of
 *                 (double)xh_p[d] over a fixed partition: pieces of 1024 consecutive members are each summed from 0.0 in
 *                 ascending member order, then the pieces are summed from 0.0 in ascending order.
 *                 EUCLID: cen'_c[d] = (float)(S_c[d] / (double)n_c).
 *                 COSINE: m = sqrt(sum_d S_c[d]^2), fp64, ascending d from 0.0, unfused; cen'_c[d] = (float)(S_c[d] / m).
 *                 n_c == 0, or m == 0 under COSINE: the centroid keeps its previous value.  No floating-point atomics.
 *   objective     fp64, over a fixed partition: O_b = the sum of (double)best[p] over p in [1024 b, 1024 (b + 1)) in ascending
 *                 p, from 0.0; objective = the sum of O_b in ascending b, from 0.0.  Larger is better.  EUCLID: with
 *                 sum_sq = the same partition sum of r_p, r_p = the fp64 sum over ascending d of the unfused (double)x_p[d]^2
 *                 taken at creation, the inertia sum_p |x_p - cen_label[p]|^2 is sum_sq - 2 * objective, up to the rounding of z.
 *   step          one assign with the current centroids, then one update.  *changed = the number of positions whose label
 *                 differs from the previous assign's (n after the first assign and after ge_kmeans_set_centroids);
 *                 *objective = that assign's.  ge_kmeans_run repeats steps until changed == 0 or max_iter steps have run.
 *   initial       a keyed sample without replacement: the K positions with the smallest (SM(seed ^ GE_KM_INIT_KEY, p), p)  (SM: the
 *   centroids     notation of the synthetic matrix above); centroid t is the prepared row of the t-th smallest: a function of
 *                 (seed, n, K) alone.  Or K centroids set by value (ge_kmeans_set_centroids): prepared like a query vector of the
 *                 nearest-neighbour index under COSINE, taken as they are under EUCLID.  There is no k-means++.
 *   bytes         labels, best scores, centroids, sizes, objective and steps are a function of the input alone, run after run.
 * Limits, checked on the host before any device work (GE_ERR_ARG without a GPU): 1 <= dim <= 1024; 1 <= k <= min(n, 65536); the
 * limits of the nearest-neighbour index on rows and subset; a known metric; max_iter >= 1; no null mandatory argument.
 * Non-finite input rows or centroids: GE_ERR_ARG ("non-finite input").  No device: GE_ERR_HIP.
 * Device memory: the prepared rows (n * D4 * 4 bytes, D4 = dim rounded up to 4), 20 bytes per row for labels, scores and the
 * member order, the sort's scratch, and (n / 1024 + k) * D4 * 8 bytes of piece sums, until ge_kmeans_destroy.
 * ---------------------------------------------------------------------------------------- */
typedef struct ge_kmeans ge_kmeans;
enum { GE_KM_COSINE = 0, GE_KM_EUCLID = 1 };
#define GE_KM_INIT_KEY 0x4B4D45414E53ull     /* "KMEANS" */
typedef struct {
    int32_t  metric;         /* GE_KM_COSINE or GE_KM_EUCLID */
    int32_t  k;              /* number of clusters */
    uint64_t seed;           /* of the initial sample */
    int32_t  device;         /* HIP device ordinal */
    void    *stream;         /* hipStream_t or NULL */
} ge_kmeans_cfg;
void      ge_kmeans_cfg_default(ge_kmeans_cfg *cfg);      /* cosine, k 0 (must be set), seed 0, device 0, null stream */
int32_t   ge_kmeans_cfg_size(void);
/* rows: HOST float[n_rows * dim], row-major; subset: NULL (every row is indexed; n_subset is ignored) or n_subset strictly
 * ascending row ids.  The handle holds the initial sample as its centroids and lives on the device until ge_kmeans_destroy. */
ge_status ge_kmeans_create(const float *rows, int64_t n_rows, int32_t dim, const int32_t *subset, int64_t n_subset,
                           const ge_kmeans_cfg *cfg, ge_kmeans **out);
/* The same on the vectors a trainer handle holds -- (focus + context) / 2, what ge_glove_extract_f32 returns -- without the
 * trip through host memory; bit for bit the handle ge_kmeans_create builds from that output.  Runs on the trainer handle's
 * device (cfg->device is ignored) and writes no trainer table. */
ge_status ge_glove_kmeans_create(ge_glove *h, const int32_t *subset, int64_t n_subset, const ge_kmeans_cfg *cfg, ge_kmeans **out);
/* centroids: HOST float[k * dim].  Starts over: steps = 0, and the next assign reports changed = n. */
ge_status ge_kmeans_set_centroids(ge_kmeans *p, const float *centroids);
/* Either out pointer may be NULL. */
ge_status ge_kmeans_step(ge_kmeans *p, int64_t *changed, double *objective);
/* *steps_run = the steps this call ran; *converged = 1 when the last of them changed no label.  Either may be NULL. */
ge_status ge_kmeans_run(ge_kmeans *p, int32_t max_iter, int32_t *steps_run, int32_t *converged);
/* Any out pointer may be NULL.  labels: HOST int32[n], best: HOST float[n], sizes: HOST int32[k] -- of the last assign, so
 * GE_ERR_STATE before the first step; centroids: HOST float[k * dim], the current ones (after the last update); *steps = the
 * steps since creation or ge_kmeans_set_centroids; *converged, *objective: of the last step (0 before the first); *sum_sq: see
 * "objective" above. */
ge_status ge_kmeans_get(const ge_kmeans *p, int64_t *n, int32_t *dim, int32_t *k, int32_t *labels, float *best, float *centroids,
                        int32_t *sizes, int32_t *steps, int32_t *converged, double *objective, double *sum_sq);
/* Device time of the last step's assign (the objective's block sums included) and update (the member sort included), hipEvents
 * around the kernels, in milliseconds (0 = none ran); copies are not counted.  Either out pointer may be NULL. */
ge_status ge_kmeans_last_kernel_ms(const ge_kmeans *p, float *assign_ms, float *update_ms);
void      ge_kmeans_destroy(ge_kmeans *p);

/* ------------------------------------------------------------------------------------------
 * Classification: given labels for some vertices, what are the labels of the rest?  Multinomial logistic (softmax) regression
 * over a table of vectors, on one device, fitted by L-BFGS.  The reference stops at the vectors file and has no counterpart,
 * so these are product semantics.  Every byte that comes back is a function of the input alone.
 *   indexed rows  as ge_kmeans_*: host rows with an optional strictly ascending subset, or the vectors of a trainer handle.
 *                 Position p = 0 .. n-1 is the p-th indexed row.  labels[p] is a class id in [0, C) or -1 (unlabelled);
 *                 train[p] is a uint8, train == NULL meaning every labelled position trains.  The training members are the
 *                 positions with labels[p] >= 0 and train[p] != 0 in ascending p: n_T >= 1 of them, member t the t-th.  A class
 *                 may have no member.
 *   features      Dp = dim + 1.  The prepared row xh_p holds dim values prepared exactly as GE_KM_COSINE (GE_CLS_COSINE, the
 *                 default) or GE_KM_EUCLID (GE_CLS_RAW) prepares them, then 1.0f at [dim], then zeros up to Dp4 = Dp rounded up
 *                 to 4.
 *   weights       W is fp32 [C][Dp], element [dim] the bias.  The master copy theta is fp64 on the host, W = (float)theta rounded
 *                 to nearest; the start is all zeros.
 *   logit         z(p, c) = the fp32 fmaf chain from +0.0f over ascending d of the Dp4 elements, s = fmaf(xh_p[d], W_c[d], s)
 *                 (k_cls_logits on the fp32 matrix cores, which give exactly that chain): the bias is the chain's last live
 *                 product.
 *   exp, log      fp64, every operation an IEEE fp64 operation, unfused, rounded to nearest even.
 *                 LN2HI = 6.93147180369123816490e-01, LN2LO = 1.90821492927058770002e-10.
 *                 cexp(t), t <= 0:  0.0 if t < -708; else k = rint(t * 1.4426950408889634), r = (t - k*LN2HI) - k*LN2LO,
 *                 p = 1/13!, then for j = 12 .. 0: p = p*r + 1/j! (each 1/j! the fp64 quotient 1.0 / (double)j!); ldexp(p, k).
 *                 clog(S), S >= 1:  (f, k) = frexp(S); if f < 0.70710678118654752440 then f = 2f, k = k - 1;
 *                 s = (f - 1)/(f + 1), w = s*s, q = 1/25, then for j = 23, 21, .. 1: q = q*w + 1/j (fp64 quotients);
 *                 k*LN2HI + (k*LN2LO + (2*s)*q).  cexp is within 1 ulp of exp on [-708, 0], clog within 3 ulp of log on
 *                 [1, 1024]; cexp(0) = 1.0, clog(1) = 0.0.
 *   softmax       of a row: m = max_c z as fp32 compares; T_c = (double)z_c - (double)m; e_c = cexp(T_c); S = the fp64 sum of
 *                 e_c from 0.0 over ascending c; q_c = e_c / S; pf_c = 0.0f if q_c < 2^-60, else (float)q_c.  For member t with
 *                 label y: the row loss l_t = clog(S) - T_y and the residuals r[t][c] = pf_c - (c == y ? 1.0f : 0.0f), one fp32
 *                 subtraction.  A non-finite logit: ge_classify_eval and ge_classify_predict fail with GE_ERR_STATE ("non-finite
 *                 logit") and leave the handle unchanged; inside ge_classify_run it is a rejected trial.
 *   loss          L = the fp64 sum of l_t over a fixed partition: blocks of 1024 members each summed from 0.0 in ascending t,
 *                 then the blocks from 0.0 in ascending order.  reg = the fp64 sum from 0.0 over ascending (c, d < dim) of the
 *                 unfused (double)W*(double)W.  f = L / (double)n_T + (0.5 * l2) * reg.
 *   gradient      pieces of 1024 consecutive members.  Gp[piece][c][d] = the fp32 fmaf chain from +0.0f over the piece's
 *                 members in ascending t of fmaf(r[t][c], xh_t[d], s) (k_cls_gradient on the fp32 matrix cores, the members
 *                 along k).  G[c][d] = the fp64 sum from 0.0 of (double)Gp over ascending pieces.
 *                 g[c*Dp + d] = G/(double)n_T + l2 * (double)W[c][d] for d < dim; the bias element is G/(double)n_T alone.
 *                 No floating-point atomics anywhere.
 *   optimiser     L-BFGS on the host in fp64, a history of 8 pairs.  dot(a, b) = the fp64 sum from 0.0 over ascending index of
 *                 the unfused products.  State: theta, f, g, the history H (pairs s, y, sy, oldest first), it.
 *                 1. max|g| <= tolerance: stop GRADIENT.  The call's max_iter iterations used up: stop MAXITER.
 *                 2. q = g; newest to oldest: a_j = dot(s_j, q) / sy_j, q -= a_j * y_j; if H is not empty,
 *                    q = (sy_new / dot(y_new, y_new)) * q; oldest to newest: b = dot(y_j, q) / sy_j, q += (a_j - b) * s_j;
 *                    d = -q, dg = dot(d, g); if !(dg < 0): empty H, d = -g, dg = dot(d, g).
 *                 3. alpha = 1.0 with history, else 1.0 / max(1.0, sqrt(dot(g, g))).  Up to 30 trials of theta' = theta + alpha*d,
 *                    (f', g') = the loss and gradient at theta'; accept when f' <= f + (1e-4 * alpha) * dg (a NaN fails);
 *                    otherwise alpha = 0.5 * alpha.  None accepted: with history, empty H and go back to 2 with the same it;
 *                    without, stop LINESEARCH.
 *                 4. s = theta' - theta, y = g' - g, sy = dot(s, y); keep the pair when sy > 1e-10 * dot(y, y), dropping the
 *                    oldest beyond 8.  Take theta', f', g'; it += 1.
 *                 The state survives between calls of ge_classify_run: run(a) then run(b) is run(a + b) unless the first stopped.
 *   prediction    for every position: label[p] = the first class in the total order of ge_nn_* (z descending as fp32 compares,
 *                 then the lower id); prob[p] = (float)(1.0 / S) (the best class has e = cexp(0) = 1.0).
 *   score         over the labelled positions p with mask[p] != 0 (mask == NULL: every labelled position), prediction against
 *                 label: integer tp, fp, fn per class and optionally the C x C confusion counts [true][predicted];
 *                 accuracy = correct / count (0 when count is 0); F1_c = 2tp / (2tp + fp + fn) in fp64; macro_f1 = the fp64
 *                 mean over ascending c of the F1_c of the classes with tp + fp + fn > 0 (0 when there is none).
 * Limits, checked on the host before any device work (GE_ERR_ARG without a GPU): 2 <= C <= 1024; labels in [-1, C); n_T >= 1;
 * n * C <= 2^33; l2 >= 0 and finite; tolerance >= 0; max_iter >= 1; finite weights; the limits of ge_kmeans_create on rows, dim
 * and subset; no null mandatory argument.  Non-finite input rows: GE_ERR_ARG ("non-finite input").  No device: GE_ERR_HIP.
 * Device memory: the prepared rows (n * Dp4 * 4 bytes), logits for max(n_T, min(n, 2^26 / C)) rows and residuals for n_T rows
 * (C * 4 bytes each), 16 bytes per member, and ceil(n_T / 1024) * C * Dp4 * 4 bytes of piece gradients, until
 * ge_classify_destroy.
 * ---------------------------------------------------------------------------------------- */
typedef struct ge_classifier ge_classifier;
enum { GE_CLS_COSINE = 0, GE_CLS_RAW = 1 };
enum { GE_CLS_STOP_NONE = 0, GE_CLS_STOP_GRADIENT = 1, GE_CLS_STOP_MAXITER = 2, GE_CLS_STOP_LINESEARCH = 3 };
typedef struct {
    int32_t  normalize;      /* GE_CLS_COSINE or GE_CLS_RAW */
    int32_t  classes;        /* C */
    double   l2;             /* weight of the penalty on the non-bias weights */
    double   tolerance;      /* on max|g| */
    int32_t  device;         /* HIP device ordinal */
    void    *stream;         /* hipStream_t or NULL */
} ge_classify_cfg;
typedef struct {
    int64_t  count, correct; /* scored positions, and those predicted right */
    double   accuracy, macro_f1;
    int64_t *tp, *fp, *fn;   /* IN: each NULL or HOST int64[C] that receives the per-class counts */
} ge_classify_summary;
void      ge_classify_cfg_default(ge_classify_cfg *cfg);  /* cosine, classes 0 (must be set), l2 1e-4, tolerance 1e-4, device 0, null stream */
int32_t   ge_classify_cfg_size(void);
/* rows: HOST float[n_rows * dim], row-major; subset as ge_kmeans_create; labels: HOST int32[n]; train: NULL or HOST uint8[n]
 * (n = the indexed rows).  The handle starts at zero weights and lives on the device until ge_classify_destroy. */
ge_status ge_classify_create(const float *rows, int64_t n_rows, int32_t dim, const int32_t *subset, int64_t n_subset,
                             const int32_t *labels, const uint8_t *train, const ge_classify_cfg *cfg, ge_classifier **out);
/* The same on the vectors a trainer handle holds -- what ge_glove_extract_f32 returns -- without the trip through host memory;
 * bit for bit the handle ge_classify_create builds from that output.  Runs on the trainer handle's device (cfg->device is
 * ignored) and writes no trainer table. */
ge_status ge_glove_classify_create(ge_glove *h, const int32_t *subset, int64_t n_subset, const int32_t *labels, const uint8_t *train,
                                   const ge_classify_cfg *cfg, ge_classifier **out);
/* weights: HOST float[C * Dp], finite.  theta = (double)weights.  Starts over: the history is emptied, iterations, evaluations
 * and the stop reason are 0 again. */
ge_status ge_classify_set_weights(ge_classifier *p, const float *weights);
/* *loss = f and grad[C * Dp] = g at the current weights: a pure read, the optimiser's state does not change.  Either may be NULL. */
ge_status ge_classify_eval(ge_classifier *p, double *loss, double *grad);
/* Up to max_iter iterations from the current state.  *iterations = the iterations this call ran; *stop = GE_CLS_STOP_*.
 * Either may be NULL. */
ge_status ge_classify_run(ge_classifier *p, int32_t max_iter, int32_t *iterations, int32_t *stop);
/* label: HOST int32[n], prob: HOST float[n], at the current weights.  Either may be NULL. */
ge_status ge_classify_predict(ge_classifier *p, int32_t *label, float *prob);
/* mask: NULL or HOST uint8[n]; confusion: NULL or HOST int64[C * C], [true][predicted].  Runs a prediction. */
ge_status ge_classify_score(ge_classifier *p, const uint8_t *mask, ge_classify_summary *summary, int64_t *confusion);
/* Any out pointer may be NULL.  weights: HOST float[C * Dp] = (float)theta; *iterations: since creation or
 * ge_classify_set_weights; *stop: of the last run (0 before it); *loss: f at theta (0 before the first run); *evaluations: the
 * loss-and-gradient evaluations ge_classify_run has made since creation or ge_classify_set_weights, the one at the starting
 * point and rejected trials included. */
ge_status ge_classify_get(const ge_classifier *p, int64_t *n, int32_t *dim, int32_t *classes, int64_t *n_train, float *weights,
                          int32_t *iterations, int32_t *stop, double *loss, int64_t *evaluations);
/* Device time of the last evaluation's logits, softmax (the loss block sums included) and gradient (the piece sums included),
 * hipEvents around the kernels, in milliseconds (0 = none ran); copies are not counted.  Any out pointer may be NULL. */
ge_status ge_classify_last_kernel_ms(const ge_classifier *p, float *logits_ms, float *softmax_ms, float *gradient_ms);
void      ge_classify_destroy(ge_classifier *p);

/* ------------------------------------------------------------------------------------------
 * Fold-in: a vector for a vertex that arrives after training.  A new row is a list of entries (id, x) against the trained
 * rows of the other side; it is fitted by the AdaGrad update of GE_ARITH_FP32 with that other side held constant.  The
 * reference has no counterpart, so these are product semantics.
 *   set        new row r, r = 0 .. n_rows-1, holds the nonzeros k in [row_ptr[r], row_ptr[r+1]), n_r of them: (idx[k], X[k]).
 *              Empty rows are legal; repeated ids inside a row are legal.
 *   frozen     GE_FOLD_FOCUS: the new rows are focus rows, b = context[idx[k]], fb_other = cBias[idx[k]].
 *   side       GE_FOLD_CONTEXT: the new rows are context rows (columns), b = focus[idx[k]], fb_other = fBias[idx[k]].
 *              Rows are read in place, where the handle keeps them, by the rules of ge_glove_eval_*: every mode, plain tables,
 *              records, packed records, a shard's focus rows counted from row_begin, bf16 rows widened exactly; for a bf16
 *              context row with hub_index[j] >= 0 the fp32 master row is read.  Nothing is staged.
 *   state      of a new row: a (D = dim floats) and fb from init_rows / init_bias, or zero; Ga = 1 for every element and
 *              Gfb = 1.  The accumulators start fresh on every run: E epochs in one run are not two runs of E / 2.
 *   update     for nonzero (b, x), always AdaGrad, whatever the handle trained with.  Every operation is an IEEE fp32 operation,
 *              rounded to nearest even, unless marked fp64; nothing is contracted beyond the fmas named under GE_ARITH_FP32.
 *              Lane shape, dot (the per-lane fmaf chain over a and b, then the tree) and the cost terms l (fp64), w with the
 *              handle's cost kind and xmax: exactly as GE_ARITH_FP32 states them.  Then
 *                ic = (float) ((double) dot + ((double) (fb + fb_other) - l));   wc = w * ic;
 *                per element  g = wc * b;   a' = a - (g / sqrtf(Ga)) * lr;   Ga' = Ga + g * g;
 *                fb' = fb - wc / sqrtf(Gfb);   Gfb' = Gfb + wc * wc;
 *              with g taken from the values read before the row changes; sqrtf and / correctly rounded.  lr = cfg.learning_rate,
 *              or the handle's when that is 0.  The lane shape defines the arithmetic, not the access width: where a row's
 *              start does not allow a vw-wide access the same elements may be read with narrower loads.  (Every layout a
 *              handle has today starts its rows on a vw-wide boundary, so the library has no narrower path; a table that
 *              broke the rule would be GE_ERR_STATE at run, never read differently.)  A dim with more than four chunks is
 *              GE_ERR_ARG.
 *   order      epochs e = 0 .. E-1.  GE_SHUFFLE_NONE: ascending k inside an epoch.  GE_SHUFFLE_DEVICE: the q-th update of epoch
 *              e is the row's B(n_r, K(0))(q)-th nonzero, B and K as under GE_MODE_STRATIFIED, K taken with iteration = e and
 *              cfg.seed.  The key does not depend on r.
 *   cost       c[r][e], fp32, from 0 per row and epoch:  c = (float) ((double) c + (0.5 * (double) wc) * (double) ic).
 *              cost_history[e] = the fp64 sum of c[r][e] over ascending r, from 0.0, computed on the host.
 *   bytes      a row's results (a, fb, c[r][.]) depend only on its own nonzeros, its init, cfg and the frozen tables: not on the
 *              other rows, its place in the set, the grid or the run.  No atomics.
 *   pure read  no trainer table is written; neither the RNG state nor the permutation is touched.  A handle that is never
 *              folded into produces the bytes it produced before.  ge_glove_fold_run may be called after any epoch and reads
 *              the tables as they are then; it runs on the trainer handle's stream and is blocking.
 * Limits, checked on the host before any device work (GE_ERR_ARG): 1 <= n_rows < 2^31; row_ptr[0] == 0 and row_ptr
 * non-decreasing; fewer than 2^31 nonzeros in all; 1 <= E <= 1024 and n_rows * E < 2^31; idx inside the frozen side's rows --
 * [0, V), or the shard's [row_begin, row_end) for GE_FOLD_CONTEXT; X finite and > 0, and < 1 for pGloVe; learning_rate 0, or
 * finite and > 0; side and shuffle known values (GE_SHUFFLE_JAVA has no per-row order); no null mandatory argument.  (What
 * needs no handle -- the null arguments, n_rows, cfg, the shape of row_ptr, ids below 0, X not finite or not positive -- is
 * refused first, so without a device as well.)  init values must be finite: a non-finite one is GE_ERR_ARG ("non-finite
 * input") at run.
 * Device memory: until ge_fold_destroy a set holds 20 bytes per nonzero (idx, l in fp64, w, x; (l, w) are computed once at
 * creation), 12 bytes per row, and 4 * n_rows * (dim + 1 + E) bytes of results.
 * ---------------------------------------------------------------------------------------- */
typedef struct ge_fold ge_fold;
enum { GE_FOLD_FOCUS = 0, GE_FOLD_CONTEXT = 1 };
typedef struct {
    int32_t side;           /* GE_FOLD_FOCUS: new rows (r, idx, x) fitted as focus rows against the frozen context rows + cBias.
                               GE_FOLD_CONTEXT: new columns (idx, r, x) fitted as context rows against the frozen focus rows + fBias */
    int32_t epochs;         /* E, 1 .. 1024 */
    int32_t shuffle;        /* GE_SHUFFLE_NONE or GE_SHUFFLE_DEVICE; GE_SHUFFLE_JAVA is GE_ERR_ARG */
    float   learning_rate;  /* 0 = the handle's */
    int64_t seed;           /* keys the DEVICE walk */
} ge_fold_cfg;
void      ge_fold_cfg_default(ge_fold_cfg *cfg);   /* focus, 10 epochs, DEVICE, lr 0, seed 0 */
int32_t   ge_fold_cfg_size(void);
/* row_ptr: HOST int64[n_rows + 1]; idx, X: HOST [row_ptr[n_rows]].  The set is uploaded once and lives on the device until
 * ge_fold_destroy. */
ge_status ge_glove_fold_create(ge_glove *h, const int64_t *row_ptr, const int32_t *idx, const float *X, int64_t n_rows,
                               const ge_fold_cfg *cfg, ge_fold **out);
/* init_rows: HOST float[n_rows * dim] or NULL (zeros); init_bias: HOST float[n_rows] or NULL (zeros).
 * out_rows float[n_rows * dim], out_bias float[n_rows], out_cost float[n_rows * E] (row-major: row r, epoch e); each may be NULL.
 * cost_history: double[E] or NULL. */
ge_status ge_glove_fold_run(ge_fold *f, const float *init_rows, const float *init_bias,
                            float *out_rows, float *out_bias, float *out_cost, double *cost_history);
/* Device time of the last run's kernel (hipEvents around it; copies not counted), in milliseconds; 0 = none ran. */
ge_status ge_fold_last_kernel_ms(const ge_fold *f, float *ms);
/* *n_rows, *nnz, *dim of the set; *path = E * the longest row.  One wavefront fits one row with every epoch inside one launch,
 * its updates strictly one after another, so the time of a run is bounded below by `path` sequential updates of the longest row
 * however many rows the set holds.  Any out pointer may be NULL. */
ge_status ge_fold_get(const ge_fold *f, int64_t *n_rows, int64_t *nnz, int32_t *dim, int64_t *path);
void      ge_fold_destroy(ge_fold *f);   /* before the ge_glove it was created for */

/* ------------------------------------------------------------------------------------------
 * Inverted-file index: top-k neighbours over the lists of the nprobe centroids closest to a query (IVF-flat), on one device.
 * Approximate only in WHICH candidates are looked at; every score, the order and every byte that comes back are exact and a
 * function of the input alone.  The reference has no counterpart, so these are product semantics.  The metric is cosine only:
 * GE_NN_DOT is GE_ERR_ARG at creation ("no quantiser for dot").
 *   indexed rows  exactly as ge_nn_create: host rows with an optional strictly ascending subset, or the vectors of a trainer
 *                 handle (ge_glove_ivf_create, bit for bit the index built from ge_glove_extract_f32's output).  Position
 *                 p = 0 .. n-1 is the p-th indexed row.  Rows are prepared as GE_NN_COSINE prepares them.
 *   centroids     L = cfg.lists of them.  TRAINED (cfg.centroids == NULL): the keyed initial sample of ge_kmeans_* with cfg.seed,
 *                 then cfg.train_iterations = T >= 0 steps of ge_kmeans_step, stopping early when a step changes no label; the
 *                 centroids after the last update are the index's, bit for bit what ge_kmeans_create + ge_kmeans_run(T) +
 *                 ge_kmeans_get(centroids) return for the same rows, GE_KM_COSINE, k = L and the same seed (the index calls that
 *                 implementation; it does not restate it).  GIVEN (cfg.centroids != NULL): HOST float[L * dim], prepared like
 *                 ge_kmeans_set_centroids prepares them; no training runs.  (Trained centroids are taken as ge_kmeans_get
 *                 returns them, not prepared again: giving them back by value reproduces the index wherever preparing a
 *                 prepared row returns its bits, which tests/test_ivf_ref.py asserts on the tables it uses.)
 *   lists         label[p] = one k-means assign against the index's centroids: the score is the fp32 fmaf chain from 0.0f over
 *                 ascending d, the winner the first c in the total order (score descending as fp32 compares, -0 = +0, NaN as
 *                 -inf, equal scores by ascending c).  List c holds the positions with label == c in ascending p.  Empty lists
 *                 are legal.
 *   probe         a query (by row id: its prepared row; by value: prepared like a query vector of ge_nn_*) is scored against
 *                 all L centroids with the same chain; its probed lists are the first nprobe centroids in that total order.
 *   candidates    C_q = the union of the probed lists, minus the query's own position under exclude_self.
 *   result        the first min(k, |C_q|) members of C_q in the total order of ge_nn_*: score descending, equal scores by
 *                 ascending ORIGINAL row id.  The score is s(q, c) as ge_nn_* defines it: the bits the exact index returns for
 *                 that pair.  out_count[q] = min(k, |C_q|); the remaining slots hold (-1, -inf); a real candidate whose score is
 *                 -inf precedes the fill.  out_candidates[q] = |C_q|.
 *   consequences  with nprobe == L the index and score arrays equal ge_nn_query_rows / ge_nn_query_vectors byte for byte.
 *                 Results do not depend on batch, grid, tile or the order in which anything arrives; there are no floating-point
 *                 atomics; the index is a pure read of a trainer handle.
 * Limits, checked on the host before any device work (GE_ERR_ARG without a GPU): the limits of ge_nn_create on rows, dim and
 * subset; 1 <= L <= min(n, 65536); 0 <= T <= 1024; 1 <= nprobe <= min(L, 128); 1 <= k <= 128; query ids that are members of the
 * index; non-finite rows, centroids or query vectors ("non-finite input"; the rows of a trainer handle are looked at on the
 * device); no null mandatory argument.  No device: GE_ERR_HIP.
 * Device memory, until ge_ivf_destroy: the table in list order (n * D4 * 4 bytes, D4 = dim rounded up to 4), 4 n bytes of
 * original row ids beside it, 4 (L + 1) bytes of list offsets and L * D4 * 4 bytes of centroids.  While ge_ivf_create runs: a
 * second copy of the table in position order (and, when it trains, what ge_kmeans_* holds, before the index allocates).
 * While a query call runs: the partial lists of a batch of queries (at most 2^24 entries of 8 bytes, or one tile of 64 queries
 * where that needs more), 24 bytes per (query, probe) pair for the schedule, and the sort's scratch.  These are allocated and
 * freed by every query call (about twenty allocations, nothing is cached between calls): a call with a handful of queries is
 * dominated by them, so send queries in large sets.  The host keeps 8 n bytes (labels and where each position sits in the
 * table).
 * ---------------------------------------------------------------------------------------- */
typedef struct ge_ivf ge_ivf;
typedef struct {
    int32_t  metric;            /* GE_NN_COSINE; GE_NN_DOT is refused */
    int32_t  lists;             /* L */
    int32_t  train_iterations;  /* T: k-means steps at most, when centroids is NULL */
    uint64_t seed;              /* of the k-means initial sample */
    const float *centroids;     /* NULL (train) or HOST float[lists * dim] */
    int32_t  device;            /* HIP device ordinal */
    void    *stream;            /* hipStream_t or NULL */
} ge_ivf_cfg;
void      ge_ivf_cfg_default(ge_ivf_cfg *cfg);            /* cosine, lists 0 (must be set), T = 10, seed 0, train, device 0 */
int32_t   ge_ivf_cfg_size(void);
/* rows, subset: as ge_nn_create.  The index lives on the device until ge_ivf_destroy. */
ge_status ge_ivf_create(const float *rows, int64_t n_rows, int32_t dim, const int32_t *subset, int64_t n_subset,
                        const ge_ivf_cfg *cfg, ge_ivf **out);
/* The same on the vectors a trainer handle holds; runs on the handle's device (cfg->device is ignored), writes no trainer table. */
ge_status ge_glove_ivf_create(ge_glove *h, const int32_t *subset, int64_t n_subset, const ge_ivf_cfg *cfg, ge_ivf **out);
/* query_ids: NULL (every indexed row, in order; n_queries must then be the number of indexed rows) or n_queries member ids.
 * out_index, out_score: HOST [n_queries * k]; out_count, out_candidates: HOST int32[n_queries].  Any out pointer may be NULL. */
ge_status ge_ivf_query_rows(ge_ivf *p, const int32_t *query_ids, int64_t n_queries, int32_t k, int32_t nprobe, int32_t exclude_self,
                            int32_t *out_index, float *out_score, int32_t *out_count, int32_t *out_candidates);
/* vectors: HOST float[n_queries * dim] */
ge_status ge_ivf_query_vectors(ge_ivf *p, const float *vectors, int64_t n_queries, int32_t k, int32_t nprobe,
                               int32_t *out_index, float *out_score, int32_t *out_count, int32_t *out_candidates);
/* Any out pointer may be NULL.  labels: HOST int32[n], by position; sizes: HOST int32[L]; centroids: HOST float[L * dim];
 * *train_steps, *converged: what ge_kmeans_run reported (0, 0 with given centroids or T = 0). */
ge_status ge_ivf_get(const ge_ivf *p, int64_t *n, int32_t *dim, int32_t *lists, int32_t *labels, int32_t *sizes, float *centroids,
                     int32_t *train_steps, int32_t *converged);
/* Device time, hipEvents around the kernels, in milliseconds (0 = none ran); copies are not counted.  build: the index's own
 * kernels at creation (prepare, assign, sort, gather; the k-means steps are ge_kmeans_*'s and not in it).  Of the last query
 * call: probe (query preparation, centroid scores, the pair sort and the schedule), scan, merge.  Any out pointer may be NULL. */
ge_status ge_ivf_last_kernel_ms(const ge_ivf *p, float *build_ms, float *probe_ms, float *scan_ms, float *merge_ms);
void      ge_ivf_destroy(ge_ivf *p);

/* ------------------------------------------------------------------------------------------
 * Matching: which rows are the same thing?  Every pair of indexed rows whose score reaches a threshold, and the groups those
 * pairs connect, on one device.  No k is chosen in advance and no number of groups.  The reference draws such edges between
 * literals at ingest (CompareJob); on the vectors it has no counterpart, so these are product semantics.
 *   indexed rows  exactly as ge_nn_create: host rows with an optional strictly ascending subset, or the vectors of a trainer
 *                 handle (ge_glove_match_create, bit for bit the index built from ge_glove_extract_f32's output).  Position
 *                 p = 0 .. n-1 is the p-th indexed row.  Prepared row as ge_nn_*: COSINE: n = sqrt(sum_d x_d^2), accumulated in
 *                 fp64 in ascending d; xh_d = (float)((double)x_d / n), rounded once; a zero row stays zero.  DOT: xh = x.
 *   score         s(a, b) = sum_d xh_a[d] * xh_b[d], an fp32 fmaf chain from +0 in ascending d (k_match_join on the fp32 matrix
 *                 cores): the bits ge_nn_* returns for that pair.  s(a, b) = s(b, a) bit for bit, because the products commute
 *                 and the order of the sum is the same.  A sum that overflows to NaN counts as -inf: it reaches no threshold.
 *   pairs         ge_match_run(p, threshold, max_pairs): all pairs of indexed rows a < b (ORIGINAL row ids) with
 *                 s(a, b) >= threshold as fp32 compares them (so -0 = +0).  A row is never paired with itself, and a pair is
 *                 listed once.  They come in ascending (a, b), each with its score bits.
 *   overflow      more than max_pairs qualifying pairs: GE_ERR_OVERFLOW.  The handle then holds no pairs and no groups;
 *                 ge_match_get's *found (and the message) carry the EXACT number of qualifying pairs, so the caller can raise
 *                 the threshold or the cap.  Exactly max_pairs qualifying pairs is not an overflow.
 *   groups        the connected components of the graph those pairs form over the indexed rows.  label[p] = the smallest
 *                 original row id in the component of indexed position p; a row without a pair labels itself.
 *   summary       pairs; components (rows without a pair included); groups = components of at least two rows; grouped_rows =
 *                 rows inside those; largest = rows of the largest component.  Integer arithmetic throughout.
 *   consequences  the bytes of a[], b[], score[], label[] and the summary are a function of the input alone: not of the grid,
 *                 the order in which workgroups arrive (it decides scratch slots only; a radix sort by (a, b) follows), the
 *                 stream, or an earlier run on the handle.  There are no floating-point atomics.  The index is a pure read of
 *                 a trainer handle.
 * Limits, checked on the host before any device work (GE_ERR_ARG without a GPU): the limits of ge_nn_create on rows, dim,
 * subset and metric; a finite threshold; 1 <= max_pairs <= 2^28; no null mandatory argument.  Non-finite input rows: GE_ERR_ARG
 * ("non-finite input").  No device: GE_ERR_HIP.  A defect inside the components kernels ends as GE_ERR_STATE, never as a kernel
 * that does not return: every loop there is bounded by n.
 * Device memory: the prepared table (n * D4 * 4 bytes, D4 = dim rounded up to 4) and 4 n bytes of row ids until
 * ge_match_destroy; while a run is under way 12 bytes per slot for min(max_pairs, n (n - 1) / 2) slots, then 20 bytes per pair
 * found and the sort's scratch, and 12 n bytes for the components.  The host keeps 12 bytes per pair and 4 n bytes of labels.
 * ---------------------------------------------------------------------------------------- */
typedef struct ge_match ge_match;
typedef struct {
    int32_t metric;          /* GE_NN_COSINE or GE_NN_DOT */
    int32_t device;          /* HIP device ordinal */
    void   *stream;          /* hipStream_t or NULL */
} ge_match_cfg;
typedef struct { int64_t pairs, components, groups, grouped_rows, largest; } ge_match_summary;
void      ge_match_cfg_default(ge_match_cfg *cfg);        /* cosine, device 0, null stream */
int32_t   ge_match_cfg_size(void);
int32_t   ge_match_summary_size(void);
/* rows, subset: as ge_nn_create.  The index lives on the device until ge_match_destroy. */
ge_status ge_match_create(const float *rows, int64_t n_rows, int32_t dim, const int32_t *subset, int64_t n_subset,
                          const ge_match_cfg *cfg, ge_match **out);
/* The same on the vectors a trainer handle holds; runs on the handle's device (cfg->device is ignored), writes no trainer table. */
ge_status ge_glove_match_create(ge_glove *h, const int32_t *subset, int64_t n_subset, const ge_match_cfg *cfg, ge_match **out);
/* One join, sort and components pass.  The threshold and max_pairs are looked at first, then the handle. */
ge_status ge_match_run(ge_match *p, float threshold, int64_t max_pairs);
/* HOST views owned by the handle, valid until the next ge_match_run or ge_match_destroy: a, b, score: [summary.pairs];
 * label: [*n_indexed], by position.  *found: the qualifying pairs of the last run (0 before the first).  Before the first run,
 * after an overflow (summary.pairs = *found then, the other fields 0) and after a failed run the views are NULL.
 * Any out pointer may be NULL. */
ge_status ge_match_get(const ge_match *p, int64_t *n_indexed, int64_t *found, const int32_t **a, const int32_t **b, const float **score,
                       const int32_t **label, ge_match_summary *summary);
/* Device time, hipEvents around the kernels, in milliseconds (0 = none ran); copies are not counted.  prepare: at creation.
 * Of the last run: join (k_match_join), sort (the radix sort and the ids), components (hook, compress, summary).
 * Any out pointer may be NULL. */
ge_status ge_match_last_kernel_ms(const ge_match *p, float *prepare_ms, float *join_ms, float *sort_ms, float *components_ms);
void      ge_match_destroy(ge_match *p);

/* ------------------------------------------------------------------------------------------
 * Alignment: which vertex of set A is which vertex of set B, each used at most once?  A rectangular join source x target above
 * a threshold, then the one-to-one assignment of a greedy walk over the candidates in descending score, on one device.  The
 * reference compares literals at ingest (CompareJob); on the vectors it has no counterpart, so these are product semantics.
 *   indexed rows  one table, taken exactly as ge_match_create takes it (host rows [n_rows][dim], or the vectors of a trainer
 *                 handle: ge_glove_align_create), and two mandatory subsets of original row ids: source (nA >= 1 ids) and
 *                 target (nB >= 1 ids), each strictly ascending and inside [0, n_rows), and disjoint from each other.  Source
 *                 position p is the p-th source id, target position q the q-th target id.  Prepared row as ge_nn_*: COSINE:
 *                 n = sqrt(sum_d x_d^2), accumulated in fp64 in ascending d; xh_d = (float)((double)x_d / n), rounded once; a
 *                 zero row stays zero.  DOT: xh = x.
 *   score         s(a, b) = sum_d xh_a[d] * xh_b[d], an fp32 fmaf chain from +0 in ascending d (k_align_join on the fp32 matrix
 *                 cores): the bits ge_nn_* and ge_match_* return for that pair.  A sum that ends as NaN counts as -inf.
 *   candidates    ge_align_run(p, threshold, max_pairs): all (a in source, b in target) with s(a, b) >= threshold as fp32
 *                 compares them, listed once each in ascending (a, b) (ORIGINAL row ids) with the score bits.
 *   overflow      more than max_pairs candidates: GE_ERR_OVERFLOW.  The handle then holds nothing; ge_align_get's *found (and
 *                 the message) carry the EXACT number of candidates.  Exactly max_pairs candidates is not an overflow.
 *   order         candidate (a, b, s) comes before (a', b', s') if s > s' as fp32 compares them (so -0 equals +0), or the scores
 *                 compare equal and a < a', or the scores compare equal, a = a' and b < b'.  A strict total order.
 *   assignment    walk the candidates in that order and accept (a, b) if neither a nor b has been accepted before.  The
 *                 accepted pairs are the alignment: no source and no target occurs twice, and no candidate is left with both
 *                 ends free.  (The device computes the same set in parallel rounds: every free vertex points at the first
 *                 candidate of its own that is still free, and a source and a target that point at each other are paired; under
 *                 a strict total order the best remaining candidate is always such a pair.)
 *   mutual        an accepted pair is mutual when b is the first candidate of a in the order and a is the first candidate of b:
 *                 the mutual-nearest-neighbour criterion.  Every such pair is accepted.
 *   outputs       a[], b[], score[]: the candidates.  By source position p: target_of[p] = the original id of the assigned
 *                 target or -1; target_score[p] = that pair's score bits, +0 where there is none; flags[p]: bit 0 = assigned,
 *                 bit 1 = mutual.  By target position q: source_of[q] = an original id or -1.
 *   summary       candidates; assigned; mutual; sources_with_candidates; targets_with_candidates; ambiguous_sources = sources
 *                 with at least two candidates.  Integer arithmetic throughout.
 *   consequences  the bytes of every output are a function of the rows, the two subsets, the metric, the threshold and max_pairs
 *                 (through the overflow rule only): not of the grid, the order in which workgroups arrive (it decides scratch
 *                 slots only; radix sorts by key follow), the stream, or an earlier run on the handle.  There are no
 *                 floating-point atomics.  The index is a pure read of a trainer handle.
 * Limits, checked on the host before any device work (GE_ERR_ARG without a GPU): the limits of ge_match_create on rows, dim
 * (1..1024), table size and metric; both subsets present, each strictly ascending and in range; "the source and target sets share
 * row %d" for a shared id; a finite threshold and 1 <= max_pairs <= 2^28 (looked at before the handle); no null mandatory
 * argument.  Non-finite input rows: GE_ERR_ARG ("non-finite input").  No device: GE_ERR_HIP.  A defect inside the assignment
 * kernels ends as GE_ERR_STATE, never as a kernel that does not return: a cursor stays inside its list, and one assigning round
 * more than min(nA, nB) stops the run.
 * Device memory: the two prepared tables ((nA + nB) * D4 * 4 bytes, D4 = dim rounded up to 4) and 4 (nA + nB) bytes of row ids
 * until ge_align_destroy; while a run is under way 12 bytes per slot for min(max_pairs, nA * nB) slots, then 56 bytes per
 * candidate and the sorts' scratch, and 29 nA + 20 nB bytes (the list starts included) for the assignment.  The
 * host keeps 12 bytes per candidate, 9 nA and 4 nB bytes.
 * ---------------------------------------------------------------------------------------- */
typedef struct ge_align ge_align;
typedef struct {
    int32_t metric;          /* GE_NN_COSINE or GE_NN_DOT */
    int32_t device;          /* HIP device ordinal */
    void   *stream;          /* hipStream_t or NULL */
} ge_align_cfg;
typedef struct { int64_t candidates, assigned, mutual, sources_with_candidates, targets_with_candidates, ambiguous_sources; } ge_align_summary;
void      ge_align_cfg_default(ge_align_cfg *cfg);        /* cosine, device 0, null stream */
int32_t   ge_align_cfg_size(void);
int32_t   ge_align_summary_size(void);
/* rows: as ge_match_create; source, target: the two sets.  The index lives on the device until ge_align_destroy. */
ge_status ge_align_create(const float *rows, int64_t n_rows, int32_t dim, const int32_t *source, int64_t n_source,
                          const int32_t *target, int64_t n_target, const ge_align_cfg *cfg, ge_align **out);
/* The same on the vectors a trainer handle holds; runs on the handle's device (cfg->device is ignored), writes no trainer table. */
ge_status ge_glove_align_create(ge_glove *h, const int32_t *source, int64_t n_source, const int32_t *target, int64_t n_target,
                                const ge_align_cfg *cfg, ge_align **out);
/* One join, the sorts and the assignment.  The threshold and max_pairs are looked at first, then the handle. */
ge_status ge_align_run(ge_align *p, float threshold, int64_t max_pairs);
/* HOST views owned by the handle, valid until the next ge_align_run or ge_align_destroy: a, b, score: [summary.candidates];
 * target_of, target_score, flags: [*n_source], by source position; source_of: [*n_target], by target position.  *found: the
 * candidates of the last run (0 before the first).  Before the first run, after an overflow (summary.candidates = *found then,
 * the other fields 0) and after a failed run the views are NULL.  Any out pointer may be NULL. */
ge_status ge_align_get(const ge_align *p, int64_t *n_source, int64_t *n_target, int64_t *found, const int32_t **a, const int32_t **b,
                       const float **score, const int32_t **target_of, const float **target_score, const uint8_t **flags,
                       const int32_t **source_of, ge_align_summary *summary);
/* Device time, hipEvents around the kernels, in milliseconds (0 = none ran); copies are not counted.  prepare: at creation.
 * Of the last run: join (k_align_join), sort (the three radix sorts, the keys and the list starts), assign (the rounds, the
 * host's looks at their counters included, the ids and the summary).  *rounds: the assignment rounds of the last run, a
 * diagnostic.  Any out pointer may be NULL. */
ge_status ge_align_last_kernel_ms(const ge_align *p, float *prepare_ms, float *join_ms, float *sort_ms, float *assign_ms, int32_t *rounds);
void      ge_align_destroy(ge_align *p);

/* ------------------------------------------------------------------------------------------ */
const char *ge_last_error(void);    /* message of the calling thread's last failed call */
const char *ge_version(void);
/* sizeof(ge_glove_cfg) as the LIBRARY was compiled: a host built against another header revision must refuse to
 * run instead of letting ge_glove_cfg_default write past its struct. */
int32_t ge_glove_cfg_size(void);
int32_t ge_glove_info_size(void);      /* sizeof(ge_glove_info), same purpose */
int32_t ge_bca_cfg_size(void);
/* Diagnostic: the rate (GB/s, bytes read + written) of a plain 16-byte-per-lane device-to-device copy of `bytes` on this
 * device -- the practical ceiling bench.py prints beside a kernel's own rate (the boxes of a pool differ). */
ge_status ge_copy_bandwidth(int32_t device, int64_t bytes, int32_t reps, double *gbps);
/* Number of visible HIP devices that are gfx950; <0 on HIP error. Does not compute. */
int32_t ge_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* GEGLOVE_H */
