/*
 * Plain-C CPU restatement of the WIDE environment: any odd 3 <= d <= 15, with the matching referee evaluated inside every step.
 *
 * TEST INFRASTRUCTURE ONLY (see oracle/__init__.py): the fast checker of csrc/env_big.hip (include/deepq_hip.h dq_envb_*) for large
 * batches.  Never linked into or called by the product library.  Restated from the Python oracle:
 *   - the environment from oracle/env_oracle.py (OracleEnv: reset / step / auto-reset, rejection loop, legal moves), with every qubit or
 *     stabilizer set an array of up to 4 x u64 and every action set ceil(num_actions / 64) words;
 *   - the referee from oracle/matching_referee.py (ComponentGraph: dist / distB / w10, the `connected` / `clusters` rule, the subset DP
 *     per cluster up to MAX_DEFECTS, the nearer-boundary fallbacks, the w10 combination, `exact`);
 *   - the state export in the layout of dq_envb_export_state.
 * PINNED: tests/test_oracle_wide_c.py (golden traces from the reference, the Python referee, the look-up referee, OracleEnv).
 *
 * Built into the same shared object as env_oracle.c (oracle/Makefile); every exported symbol starts with dqw_.
 */
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef uint64_t u64;
typedef uint32_t u32;
typedef uint8_t u8;

#define W_MAX 4                          /* words of a qubit / stabilizer set: d^2 <= 225                     */
#define LW_MAX 11                        /* words of an action set: 3 d^2 + 1 <= 676                         */
#define D_MAX 15
#define Q_MAX (D_MAX * D_MAX)
#define S_MAX (Q_MAX - 1)
#define N_MAX 112                        /* plaquettes per component: (d^2 - 1) / 2                          */
#define DEPTH_MAX 16

#define MAX_DEFECTS 20                   /* per cluster (oracle/matching_referee.py)                          */
#define MAX_LIST 32                      /* defects of a component that are listed and clustered              */
#define INF 255
#define BIG (1 << 20)

/* ------------------------------------------------------------------------------------------
 * Philox4x32-10 (oracle/philox.py)
 * ---------------------------------------------------------------------------------------- */
static void philox(u32 c0, u32 c1, u32 c2, u32 c3, const u32 key[2], u32 out[4]) {
    u32 k0 = key[0], k1 = key[1];
    for (int r = 0; r < 10; ++r) {
        u64 p0 = (u64)0xD2511F53u * c0, p1 = (u64)0xCD9E8D57u * c2;
        u32 n0 = (u32)(p1 >> 32) ^ c1 ^ k0, n1 = (u32)p1, n2 = (u32)(p0 >> 32) ^ c3 ^ k1, n3 = (u32)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

static inline void bset(u64* m, int i) { m[i >> 6] |= 1ull << (i & 63); }
static inline int bget(const u64* m, int i) { return (int)((m[i >> 6] >> (i & 63)) & 1); }

/* ------------------------------------------------------------------------------------------
 * Lattice tables (oracle/lattice.py)
 * ---------------------------------------------------------------------------------------- */
static int ptype(int d, int a, int b) {
    if ((a == 0 && b % 2 == 0) || (a == d && b % 2 == 1) || (b == 0 && a % 2 == 1) || (b == d && a % 2 == 0)) return 0;
    return ((a + b) & 1) ? 3 : 1;
}

typedef struct {
    int d, d2, n_stab, W;
    int stab_a[S_MAX], stab_b[S_MAX], stab_type[S_MAX];
    int node[S_MAX];                     /* stabilizer -> its index in its own type's row-major order (the referee index bit)  */
    u64 stab_q[S_MAX][W_MAX];            /* qubits of stabilizer s                                                            */
    u64 qubit_s[Q_MAX][W_MAX];           /* live stabilizers touched by qubit q (ENV:262-271)                                 */
    u64 neigh[Q_MAX][W_MAX];             /* 8-neighbourhood of qubit q (ENV:349-372)                                          */
    u64 col0[W_MAX], row0[W_MAX];
    u8 static_plane[(2 * D_MAX + 1) * (2 * D_MAX + 1)];
} wlattice;

static void wlattice_init(wlattice* L, int d) {
    memset(L, 0, sizeof(*L));
    L->d = d; L->d2 = d * d; L->n_stab = d * d - 1; L->W = (d * d + 63) / 64;
    int s = 0, half = (d + 1) / 2 - 1;
    for (int a = 1; a < d; ++a) for (int b = 1; b < d; ++b) { L->stab_a[s] = a; L->stab_b[s] = b; ++s; }
    for (int x = 0; x < half; ++x) { L->stab_a[s] = 0; L->stab_b[s] = 2 * x + 1; ++s; }
    for (int x = 0; x < half; ++x) { L->stab_a[s] = d; L->stab_b[s] = 2 * x + 2; ++s; }
    for (int x = 0; x < half; ++x) { L->stab_a[s] = 2 * x + 2; L->stab_b[s] = 0; ++s; }
    for (int x = 0; x < half; ++x) { L->stab_a[s] = 2 * x + 1; L->stab_b[s] = d; ++s; }
    for (s = 0; s < L->n_stab; ++s) {
        int a = L->stab_a[s], b = L->stab_b[s];
        L->stab_type[s] = ptype(d, a, b);
        /* rank among the plaquettes of the same type in row-major (a, b) order */
        int r = 0;
        for (int aa = 0; aa <= d; ++aa) for (int bb = 0; bb <= d; ++bb)
            if ((aa < a || (aa == a && bb < b)) && ptype(d, aa, bb) == L->stab_type[s]) ++r;
        L->node[s] = r;
        for (int x = a - 1; x <= a; ++x) for (int y = b - 1; y <= b; ++y)
            if (x >= 0 && x < d && y >= 0 && y < d) {
                bset(L->stab_q[s], x * d + y);
                bset(L->qubit_s[x * d + y], s);
            }
    }
    for (int r = 0; r < d; ++r) for (int c = 0; c < d; ++c)
        for (int dr = -1; dr <= 1; ++dr) for (int dc = -1; dc <= 1; ++dc) {
            int rr = r + dr, cc = c + dc;
            if ((dr || dc) && rr >= 0 && rr < d && cc >= 0 && cc < d) bset(L->neigh[r * d + c], rr * d + cc);
        }
    for (int x = 0; x < d; ++x) bset(L->col0, x * d);
    for (int y = 0; y < d; ++y) bset(L->row0, y);
    int n = 2 * d + 1;
    for (int x = 0; x < n; ++x) for (int y = 0; y < n; ++y) {
        u8 v = 0;
        if ((x == 0 || x == n - 1) && (y & 1)) v = 1;
        if ((y == 0 || y == n - 1) && (x & 1)) v = 1;
        if ((x & 1) && (y & 1) && ((x + y) % 4 == 0)) v = 1;
        L->static_plane[x * n + y] = v;
    }
}

static void syndrome(const wlattice* L, const u64* xm, const u64* zm, u64* out) {
    for (int w = 0; w < W_MAX; ++w) out[w] = 0;
    for (int s = 0; s < L->n_stab; ++s) {
        const u64* comp = L->stab_type[s] == 3 ? xm : zm;
        int par = 0;
        for (int w = 0; w < L->W; ++w) par += __builtin_popcountll(comp[w] & L->stab_q[s][w]);
        if (par & 1) bset(out, s);
    }
}

/* ------------------------------------------------------------------------------------------
 * Matching referee (oracle/matching_referee.py ComponentGraph / MatchingReferee)
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int d, typ, n, w10;
    u8 dist[N_MAX][N_MAX][2];
    u8 distB[N_MAX][2];
    int deg[N_MAX];
    int adj_to[N_MAX][4], adj_lg[N_MAX][4];        /* other node, or -1 for the boundary; logical bit */
} wgraph;

static void wgraph_init(wgraph* G, const wlattice* L, int typ) {
    memset(G, 0, sizeof(*G));
    int d = L->d;
    G->d = d; G->typ = typ;
    int pos[D_MAX + 1][D_MAX + 1];
    int n = 0;
    for (int a = 0; a <= d; ++a) for (int b = 0; b <= d; ++b) pos[a][b] = ptype(d, a, b) == typ ? n++ : -1;
    G->n = n;
    for (int x = 0; x < d; ++x) for (int y = 0; y < d; ++y) {
        int ends[4], ne = 0;
        const int ab[4][2] = {{x, y}, {x, y + 1}, {x + 1, y}, {x + 1, y + 1}};
        for (int k = 0; k < 4; ++k) if (pos[ab[k][0]][ab[k][1]] >= 0) ends[ne++] = pos[ab[k][0]][ab[k][1]];
        /* (the Python graph orders the two ends by node index) */
        if (ne == 2 && ends[0] > ends[1]) { int t = ends[0]; ends[0] = ends[1]; ends[1] = t; }
        int lg = typ == 3 ? (y == 0) : (x == 0);
        if (ne == 2) {
            G->adj_to[ends[0]][G->deg[ends[0]]] = ends[1]; G->adj_lg[ends[0]][G->deg[ends[0]]++] = lg;
            G->adj_to[ends[1]][G->deg[ends[1]]] = ends[0]; G->adj_lg[ends[1]][G->deg[ends[1]]++] = lg;
        } else if (ne == 1) {
            G->adj_to[ends[0]][G->deg[ends[0]]] = -1; G->adj_lg[ends[0]][G->deg[ends[0]]++] = lg;
        } else {
            abort();
        }
    }
    memset(G->dist, INF, sizeof(G->dist));
    memset(G->distB, INF, sizeof(G->distB));
    int fr[2 * N_MAX], nx[2 * N_MAX];
    for (int u = 0; u < n; ++u) {                                 /* breadth-first search over (node, class), never through the boundary */
        u8 seen[N_MAX][2];
        memset(seen, 0, sizeof(seen));
        seen[u][0] = 1;
        G->dist[u][u][0] = 0;
        int nf = 0, w = 0;
        fr[nf++] = 2 * u;
        while (nf) {
            ++w;
            int nn = 0;
            for (int f = 0; f < nf; ++f) {
                int x = fr[f] >> 1, c = fr[f] & 1;
                for (int k = 0; k < G->deg[x]; ++k) {
                    int y = G->adj_to[x][k], c2 = c ^ G->adj_lg[x][k];
                    if (y < 0) {
                        if (G->distB[u][c2] == INF) G->distB[u][c2] = (u8)w;
                    } else if (!seen[y][c2]) {
                        seen[y][c2] = 1;
                        G->dist[u][y][c2] = (u8)w;
                        nx[nn++] = 2 * y + c2;
                    }
                }
            }
            memcpy(fr, nx, nn * sizeof(int));
            nf = nn;
        }
    }
    int w10 = INF;
    for (int u = 0; u < n; ++u) {
        for (int k = 0; k < G->deg[u]; ++k)
            if (G->adj_to[u][k] < 0) {
                int v = 1 + (int)G->distB[u][1 ^ G->adj_lg[u][k]];
                if (v < w10) w10 = v;
            }
        if ((int)G->dist[u][u][1] < w10) w10 = G->dist[u][u][1];
    }
    G->w10 = w10 < INF ? w10 : INF;
}

static inline int dB(const wgraph* G, int u, int c) { return G->distB[u][c] == INF ? BIG : G->distB[u][c]; }
static inline int dD(const wgraph* G, int u, int v, int c) { return G->dist[u][v][c] == INF ? BIG : G->dist[u][v][c]; }
static inline int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }

/* ComponentGraph._dp: the subset DP level by level of the subsets' highest defect */
static void wdp(const wgraph* G, const int* core, int k, int64_t out[2]) {
    int32_t* f = (int32_t*)malloc(sizeof(int32_t) * 2 * ((size_t)1 << k));
    if (!f) abort();
    f[0] = 0; f[1] = BIG;
    for (int h = 0; h < k; ++h) {
        const int base = 1 << h, u = core[h];
        const int64_t b0 = dB(G, u, 0), b1 = dB(G, u, 1);
        int64_t d0[MAX_DEFECTS], d1[MAX_DEFECTS];
        for (int v = 0; v < h; ++v) { d0[v] = dD(G, u, core[v], 0); d1[v] = dD(G, u, core[v], 1); }
        for (int r = 0; r < base; ++r) {
            int64_t g0 = f[2 * r], g1 = f[2 * r + 1];
            int64_t best0 = min64(g0 + b0, g1 + b1), best1 = min64(g1 + b0, g0 + b1);
            for (unsigned m = (unsigned)r; m; m &= m - 1) {           /* every v < h in the subset r */
                int v = __builtin_ctz(m), rr = r ^ (1 << v);
                int64_t q0 = f[2 * rr], q1 = f[2 * rr + 1];
                best0 = min64(best0, min64(q0 + d0[v], q1 + d1[v]));
                best1 = min64(best1, min64(q1 + d0[v], q0 + d1[v]));
            }
            f[2 * (base + r)] = (int32_t)min64(best0, BIG);
            f[2 * (base + r) + 1] = (int32_t)min64(best1, BIG);
        }
    }
    size_t last = ((size_t)1 << k) - 1;
    out[0] = f[2 * last]; out[1] = f[2 * last + 1];
    free(f);
}

/* ComponentGraph._to_boundary: every defect of `extra` to its nearer boundary, ties -> the class-0 path */
static void wto_boundary(const wgraph* G, int64_t w[2], const int* extra, int n) {
    for (int i = 0; i < n; ++i) {
        int u = extra[i];
        int cp = G->distB[u][1] < G->distB[u][0] ? 1 : 0;
        int64_t add = G->distB[u][cp];
        int64_t a = w[cp] + add, b = w[1 ^ cp] + add;
        w[0] = a; w[1] = b;
    }
}

static int wconnected(const wgraph* G, int u, int v) {
    for (int cp = 0; cp < 2; ++cp) {
        if (G->dist[u][v][cp] == INF) continue;
        int a = dB(G, u, 0) + dB(G, v, cp), b = dB(G, u, 1) + dB(G, v, 1 ^ cp);
        if ((int)G->dist[u][v][cp] < (a < b ? a : b)) return 1;
    }
    return 0;
}

/* ComponentGraph.weights for an ascending defect list.  flags: bit 0 a cluster beyond MAX_DEFECTS, bit 1 defects beyond MAX_LIST. */
static void wweights(const wgraph* G, const int* defects, int nd, int64_t out[2], int* flags) {
    int listed = nd < MAX_LIST ? nd : MAX_LIST;
    int fl = nd > MAX_LIST ? 2 : 0;
    int comp[MAX_LIST];
    for (int i = 0; i < listed; ++i) comp[i] = i;
    int changed = 1;
    while (changed) {                                              /* label propagation to the component's lowest index */
        changed = 0;
        for (int i = 0; i < listed; ++i) {
            int m = comp[i];
            for (int j = 0; j < listed; ++j)
                if (j != i && wconnected(G, defects[i], defects[j]) && comp[j] < m) m = comp[j];
            if (m != comp[i]) { comp[i] = m; changed = 1; }
        }
    }
    int64_t w[2] = {0, BIG};
    for (int r = 0; r < listed; ++r) {
        if (comp[r] != r) continue;
        int cl[MAX_LIST], k = 0;
        for (int i = 0; i < listed; ++i) if (comp[i] == r) cl[k++] = defects[i];
        int64_t wc[2];
        wdp(G, cl, k < MAX_DEFECTS ? k : MAX_DEFECTS, wc);
        if (k > MAX_DEFECTS) { wto_boundary(G, wc, cl + MAX_DEFECTS, k - MAX_DEFECTS); fl |= 1; }
        int64_t n0 = min64(min64(w[0] + wc[0], w[1] + wc[1]), BIG), n1 = min64(min64(w[0] + wc[1], w[1] + wc[0]), BIG);
        w[0] = n0; w[1] = n1;
    }
    if (nd > listed) wto_boundary(G, w, defects + listed, nd - listed);
    out[0] = min64(w[0], w[1] + G->w10);
    out[1] = min64(w[1], w[0] + G->w10);
    *flags = fl;
}

/* class of one component's syndrome given as node bits (bit i = the i-th plaquette of the component's row-major order) */
static int wclassify_bits(const wgraph* G, const u64 bits[2], int64_t w[2], int* flags) {
    int defects[N_MAX], nd = 0;
    for (int i = 0; i < G->n; ++i) if ((bits[i >> 6] >> (i & 63)) & 1) defects[nd++] = i;
    int64_t ww[2];
    wweights(G, defects, nd, ww, flags);
    if (w) { w[0] = ww[0]; w[1] = ww[1]; }
    return ww[1] < ww[0];
}

typedef struct {
    wlattice L;
    wgraph g[2];                         /* 0: type-3 plaquettes (X part), 1: type-1 plaquettes (Z part) */
} dqw_match;

dqw_match* dqw_match_create(int d) {
    if (d < 3 || d > D_MAX || !(d & 1)) return NULL;
    dqw_match* M = (dqw_match*)calloc(1, sizeof(dqw_match));
    if (!M) return NULL;
    wlattice_init(&M->L, d);
    wgraph_init(&M->g[0], &M->L, 3);
    wgraph_init(&M->g[1], &M->L, 1);
    return M;
}

void dqw_match_destroy(dqw_match* M) { free(M); }

/* tables of one component, for tests: dist uint8 [n][n][2], distB uint8 [n][2]; returns n, *w10 */
int dqw_match_tables(const dqw_match* M, int comp, u8* dist, u8* distB, int* w10) {
    const wgraph* G = &M->g[comp];
    for (int u = 0; u < G->n; ++u) {
        for (int v = 0; v < G->n; ++v) { dist[(u * G->n + v) * 2] = G->dist[u][v][0]; dist[(u * G->n + v) * 2 + 1] = G->dist[u][v][1]; }
        distB[2 * u] = G->distB[u][0]; distB[2 * u + 1] = G->distB[u][1];
    }
    *w10 = G->w10;
    return G->n;
}

/* batch over syndromes of one component: bits uint64 [n][2]; cls uint8 [n]; w int64 [n][2] (nullable); flags uint8 [n] (nullable) */
void dqw_match_classify(const dqw_match* M, int comp, const u64* bits, int n, u8* cls, int64_t* w, u8* flags) {
    for (int i = 0; i < n; ++i) {
        int fl;
        int64_t ww[2];
        cls[i] = (u8)wclassify_bits(&M->g[comp], bits + 2 * (size_t)i, ww, &fl);
        if (w) { w[2 * i] = ww[0]; w[2 * i + 1] = ww[1]; }
        if (flags) flags[i] = (u8)fl;
    }
}

/* ------------------------------------------------------------------------------------------
 * Batched wide environment
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    u64 x[W_MAX], z[W_MAX], acted[W_MAX], round;
    u64 volume[DEPTH_MAX][W_MAX];
    u64 completed[LW_MAX], legal[LW_MAX];
    u32 lifetime;
    u8 done;
} wstate;

typedef struct {
    dqw_match M;
    int model, use_Y, depth, layers, n_actions, identity, C, n_envs, LW, threads;
    u32 seed[2], env_id_base;
    u64 T_phys, T_meas;
    wstate* st;
} dqw_env;

static u64 rate_threshold(double p) {   /* W/2^32 < p  <=>  W < ceil(p*2^32) */
    double t = p * 4294967296.0;
    if (t <= 0.0) return 0;
    if (t >= 4294967296.0) return 1ull << 32;
    u64 f = (u64)t;
    return ((double)f < t) ? f + 1 : f;
}

dqw_env* dqw_env_create(int d, int model, int use_Y, int depth, int n_envs, u32 env_id_base, u32 seed0, u32 seed1) {
    if (d < 3 || d > D_MAX || !(d & 1) || depth < 1 || depth > DEPTH_MAX || n_envs < 1 || model < 0 || model > 2) return NULL;
    dqw_env* E = (dqw_env*)calloc(1, sizeof(dqw_env));
    if (!E) return NULL;
    wlattice_init(&E->M.L, d);
    wgraph_init(&E->M.g[0], &E->M.L, 3);
    wgraph_init(&E->M.g[1], &E->M.L, 1);
    E->model = model; E->use_Y = use_Y; E->depth = depth; E->n_envs = n_envs;
    E->layers = model == 0 ? 1 : (use_Y ? 3 : 2);
    E->n_actions = E->layers * d * d + 1;
    E->identity = E->n_actions - 1;
    E->LW = (E->n_actions + 63) / 64;
    E->C = depth + E->layers;
    E->seed[0] = seed0; E->seed[1] = seed1; E->env_id_base = env_id_base;
    E->st = (wstate*)calloc(n_envs, sizeof(wstate));
    if (!E->st) { free(E); return NULL; }
    return E;
}

void dqw_env_destroy(dqw_env* E) { if (E) { free(E->st); free(E); } }
/* reset / step run lattices [i * n / threads, (i + 1) * n / threads) on thread i: lattices are independent, so results do not depend on it */
void dqw_env_set_threads(dqw_env* E, int threads) { E->threads = threads < 1 ? 1 : (threads > 64 ? 64 : threads); }
void dqw_env_set_rates(dqw_env* E, double p_phys, double p_meas) { E->T_phys = rate_threshold(p_phys); E->T_meas = rate_threshold(p_meas); }
int dqw_env_num_actions(const dqw_env* E) { return E->n_actions; }
int dqw_env_legal_words(const dqw_env* E) { return E->LW; }
int dqw_env_obs_size(const dqw_env* E) { int n = 2 * E->M.L.d + 1; return E->C * n * n; }
int dqw_env_state_words(const dqw_env* E) { return 5 * E->M.L.W + 2 + 2 * E->LW + E->depth * E->M.L.W; }

static void new_volume(dqw_env* E, wstate* S, u32 env_id) {          /* OracleEnv._new_volume */
    const wlattice* L = &E->M.L;
    u64 summed_any;
    do {
        summed_any = 0;
        for (int j = 0; j < E->depth; ++j) {
            u64 ex[W_MAX] = {0}, ez[W_MAX] = {0}, fl[W_MAX] = {0}, tw[W_MAX];
            for (int lane = 0; lane < L->d2; ++lane) {                /* OracleEnv._draw_round */
                u32 w[4];
                philox((u32)S->round, (u32)(S->round >> 32), env_id, (u32)lane, E->seed, w);
                if (E->model == 2) {
                    if ((u64)w[0] < E->T_phys) bset(ex, lane);
                    if ((u64)w[1] < E->T_phys) bset(ez, lane);
                } else if ((u64)w[0] < E->T_phys) {
                    int t = E->model == 0 ? 1 : 1 + (int)(((u64)w[1] * 3) >> 32);
                    if (t == 1 || t == 2) bset(ex, lane);
                    if (t == 2 || t == 3) bset(ez, lane);
                }
                if (lane < L->n_stab && (u64)w[2] < E->T_meas) bset(fl, lane);
            }
            S->round++;
            for (int w = 0; w < L->W; ++w) { S->x[w] ^= ex[w]; S->z[w] ^= ez[w]; }
            syndrome(L, S->x, S->z, tw);
            for (int w = 0; w < L->W; ++w) { S->volume[j][w] = tw[w] ^ fl[w]; summed_any |= S->volume[j][w]; }
            S->lifetime++;
        }
    } while (!summed_any);
}

static void reset_legal(dqw_env* E, wstate* S) {                      /* OracleEnv._reset_legal_moves */
    const wlattice* L = &E->M.L;
    u64 summed[W_MAX] = {0};
    for (int j = 0; j < E->depth; ++j) for (int w = 0; w < L->W; ++w) summed[w] |= S->volume[j][w];
    memset(S->completed, 0, sizeof(S->completed));
    memset(S->acted, 0, sizeof(S->acted));
    memset(S->legal, 0, sizeof(S->legal));
    bset(S->legal, E->identity);
    for (int q = 0; q < L->d2; ++q) {
        u64 touch = 0;
        for (int w = 0; w < L->W; ++w) touch |= L->qubit_s[q][w] & summed[w];
        if (touch) for (int j = 0; j < E->layers; ++j) bset(S->legal, q + j * L->d2);
    }
}

static void write_obs(const dqw_env* E, const wstate* S, u8* obs) {
    const wlattice* L = &E->M.L;
    int n = 2 * L->d + 1, plane = n * n;
    for (int j = 0; j < E->depth; ++j) {
        u8* p = obs + j * plane;
        memcpy(p, L->static_plane, plane);
        for (int s = 0; s < L->n_stab; ++s) p[2 * L->stab_a[s] * n + 2 * L->stab_b[s]] = (u8)bget(S->volume[j], s);
    }
    for (int k = 0; k < E->layers; ++k) {
        u8* p = obs + (E->depth + k) * plane;
        memset(p, 0, plane);
        for (int q = 0; q < L->d2; ++q)
            if (bget(S->completed, k * L->d2 + q)) p[(2 * (q / L->d) + 1) * n + 2 * (q % L->d) + 1] = 1;
    }
}

static void env_reset_one(dqw_env* E, wstate* S, u32 env_id) {         /* OracleEnv.reset */
    S->done = 0; S->lifetime = 0;
    memset(S->x, 0, sizeof(S->x)); memset(S->z, 0, sizeof(S->z));
    new_volume(E, S, env_id);
    reset_legal(E, S);
}

/* the referee on the true syndrome (MatchingReferee.classify_word); *inexact: a fallback was used */
static int referee(const dqw_env* E, const u64* tw, int* inexact) {
    const wlattice* L = &E->M.L;
    u64 bits[2][2] = {{0, 0}, {0, 0}};
    for (int s = 0; s < L->n_stab; ++s)
        if (bget(tw, s)) { int c = L->stab_type[s] == 3 ? 0 : 1; bits[c][L->node[s] >> 6] |= 1ull << (L->node[s] & 63); }
    int fl = 0, f2 = 0;
    int dec = wclassify_bits(&E->M.g[0], bits[0], NULL, &fl);
    if (E->model != 0) dec += 2 * wclassify_bits(&E->M.g[1], bits[1], NULL, &f2);
    *inexact = (fl | f2) != 0;
    return dec;
}

static float env_step_one(dqw_env* E, wstate* S, u32 env_id, int action, int* inexact) {   /* OracleEnv.step */
    const wlattice* L = &E->M.L;
    if (action < 0 || action >= E->n_actions) action = E->identity;
    int done_identity = action == E->identity || bget(S->completed, action);
    if (action < E->layers * L->d2) {
        int layer = action / L->d2, q = action % L->d2;
        int pauli = E->model == 0 ? 1 : (E->use_Y ? layer + 1 : (layer == 0 ? 1 : 3));
        if (pauli == 1 || pauli == 2) S->x[q >> 6] ^= 1ull << (q & 63);
        if (pauli == 2 || pauli == 3) S->z[q >> 6] ^= 1ull << (q & 63);
    }
    u64 tw[W_MAX];
    syndrome(L, S->x, S->z, tw);
    int px = 0, pz = 0;
    u64 any = 0;
    for (int w = 0; w < L->W; ++w) {
        px += __builtin_popcountll(S->x[w] & L->col0[w]);
        pz += __builtin_popcountll(S->z[w] & L->row0[w]);
        any |= tw[w];
    }
    int correct = (px & 1) + 2 * (pz & 1);
    int decoded = referee(E, tw, inexact);
    float reward = 0.f;
    if (correct == 0 && !any) reward = 1.f;
    else if (decoded != correct) S->done = 1;
    if (done_identity) {
        new_volume(E, S, env_id);
        reset_legal(E, S);
    } else {
        bset(S->completed, action);
        int q = action % L->d2;
        if (!bget(S->acted, q)) {
            bset(S->acted, q);
            for (int j = 0; j < E->layers; ++j)
                for (int nb = 0; nb < L->d2; ++nb)
                    if (bget(L->neigh[q], nb)) bset(S->legal, nb + j * L->d2);
        }
    }
    return reward;
}

static void emit(const dqw_env* E, const wstate* S, int i, u8* obs, u8* done, u64* legal, u32* lifetime) {
    if (obs) write_obs(E, S, obs + (size_t)i * dqw_env_obs_size(E));
    if (done) done[i] = S->done;
    if (legal) for (int k = 0; k < E->LW; ++k) legal[(size_t)i * E->LW + k] = S->legal[k];
    if (lifetime) lifetime[i] = S->lifetime;
}

typedef struct {
    dqw_env* E;
    int lo, hi, mode, auto_reset;        /* mode 0: reset, 1: step */
    const u8* which;
    const int32_t* action;
    u8 *obs, *done, *was_reset, *inexact;
    float* reward;
    u64* legal;
    u32* lifetime;
} wjob;

static void* run_job(void* arg) {
    wjob* J = (wjob*)arg;
    dqw_env* E = J->E;
    for (int i = J->lo; i < J->hi; ++i) {
        wstate* S = &E->st[i];
        const u32 id = E->env_id_base + (u32)i;
        if (J->mode == 0) {
            if (!J->which || J->which[i]) env_reset_one(E, S, id);
            emit(E, S, i, J->obs, NULL, J->legal, J->lifetime);
            continue;
        }
        float r = 0.f;
        int wr = 0, ix = 0;
        if (J->auto_reset && S->done) { env_reset_one(E, S, id); wr = 1; }
        else r = env_step_one(E, S, id, J->action[i], &ix);
        if (J->reward) J->reward[i] = r;
        if (J->was_reset) J->was_reset[i] = (u8)wr;
        if (J->inexact) J->inexact[i] = (u8)ix;
        emit(E, S, i, J->obs, J->done, J->legal, J->lifetime);
    }
    return NULL;
}

static void run_all(const wjob* proto) {
    dqw_env* E = proto->E;
    int T = E->threads < 1 ? 1 : E->threads;
    if (T > E->n_envs) T = E->n_envs;
    wjob jobs[64];
    pthread_t tid[64];
    int started[64] = {0};
    for (int t = 0; t < T; ++t) {
        jobs[t] = *proto;
        jobs[t].lo = (int)((long long)E->n_envs * t / T);
        jobs[t].hi = (int)((long long)E->n_envs * (t + 1) / T);
        if (t > 0) started[t] = pthread_create(&tid[t], NULL, run_job, &jobs[t]) == 0;
    }
    run_job(&jobs[0]);
    for (int t = 1; t < T; ++t) {
        if (started[t]) pthread_join(tid[t], NULL);
        else run_job(&jobs[t]);                                       /* no thread to be had: do the slice here */
    }
}

/* which == NULL: reset all; else reset env i iff which[i] != 0 (others untouched but still emitted) */
void dqw_env_reset(dqw_env* E, const u8* which, u8* obs, u64* legal, u32* lifetime) {
    wjob J = {E, 0, 0, 0, 0, which, NULL, obs, NULL, NULL, NULL, NULL, legal, lifetime};
    run_all(&J);
}

/* auto_reset: an env whose done flag is set when the call starts is reset instead of stepped (action ignored, reward 0, inexact 0) */
void dqw_env_step(dqw_env* E, const int32_t* action, int auto_reset, u8* obs, float* reward, u8* done,
                  u64* legal, u32* lifetime, u8* was_reset, u8* inexact) {
    wjob J = {E, 0, 0, 1, auto_reset, NULL, action, obs, done, was_reset, inexact, reward, legal, lifetime};
    run_all(&J);
}

/* dq_envb_export_state's layout per env: x[W] z[W] true_syndrome[W] summed[W] acted[W] round completed[LW] legal[LW]
 * (lifetime | done << 32) volume[depth][W] */
void dqw_env_export(const dqw_env* E, u64* out) {
    const wlattice* L = &E->M.L;
    const int W = L->W, LW = E->LW, sw = dqw_env_state_words(E);
    for (int i = 0; i < E->n_envs; ++i) {
        const wstate* S = &E->st[i];
        u64* o = out + (size_t)i * sw;
        u64 tw[W_MAX], summed[W_MAX] = {0};
        syndrome(L, S->x, S->z, tw);
        for (int j = 0; j < E->depth; ++j) for (int w = 0; w < W; ++w) summed[w] |= S->volume[j][w];
        for (int w = 0; w < W; ++w) { o[w] = S->x[w]; o[W + w] = S->z[w]; o[2 * W + w] = tw[w]; o[3 * W + w] = summed[w]; o[4 * W + w] = S->acted[w]; }
        o[5 * W] = S->round;
        for (int k = 0; k < LW; ++k) { o[5 * W + 1 + k] = S->completed[k]; o[5 * W + 1 + LW + k] = S->legal[k]; }
        o[5 * W + 1 + 2 * LW] = (u64)S->lifetime | ((u64)S->done << 32);
        for (int j = 0; j < E->depth; ++j) for (int w = 0; w < W; ++w) o[5 * W + 2 + 2 * LW + j * W + w] = S->volume[j][w];
    }
}

/* uniform over the legal set from the POLICY stream (the rule of policy_wide_kernel): word 0 of
 * Philox(key=seed, ctr=(t_lo, t_hi, env_id, 1 << 16)); k = (w * n_legal) >> 32; the k-th set bit over all LW words */
void dqw_policy_uniform_legal(const dqw_env* E, u64 t, const u64* legal, int32_t* action) {
    for (int i = 0; i < E->n_envs; ++i) {
        u32 w[4];
        philox((u32)t, (u32)(t >> 32), E->env_id_base + (u32)i, 1u << 16, E->seed, w);
        const u64* lg = legal + (size_t)i * E->LW;
        int n = 0;
        for (int k = 0; k < E->LW; ++k) n += __builtin_popcountll(lg[k]);
        int kk = (int)(((u64)w[0] * (u64)n) >> 32), a = -1;
        for (int b = 0; b < 64 * E->LW; ++b)
            if (bget(lg, b) && kk-- == 0) { a = b; break; }
        action[i] = a;
    }
}
