/*
 * mvx_graph.c -- HIP graphs of device calls (mvx_comm_set_graphs): the cache
 * of captured jobs and its key, capture, launch, replay, and when a captured
 * graph is destroyed.  What a call issues is mvx_exec.c's
 * (mvxi_run_device_eager); here it is issued as it comes, captured or
 * replayed.
 *
 * The first call of a job runs eagerly (it also sizes the staging pool and
 * opens RCCL's connections); the second is captured into a HIP graph on the
 * call's stream -- RCCL's groups record their kernels, PIPE's combine stream
 * joins through its events -- and launched; later ones replay it.  A
 * capture that fails turns graphs off on the communicator (graph_error) and
 * the call runs eagerly.  Null-stream calls capture and replay on the
 * communicator's own stream (mvxi_null_fork / mvxi_null_join, mvx_exec.c).
 *
 * A captured graph is destroyed with its communicator (mvxi_graphs_clear,
 * before ncclCommDestroy), and mid-life where the runtime allows it
 * (graph_evictable): before the staging pool it was captured on is freed
 * (mvxi_graphs_unpool), and as the least recently used one when every slot
 * holds a graph and a job seen twice is about to be captured.  The runtime
 * allows any graph from HIP 7.2 on and only single-branch ones before it
 * (PIPE's forked captures are not).  A graph that may not be destroyed when
 * its pool goes is retired: kept, never matched again.  Where no slot is
 * free and no graph may be evicted, new jobs run eagerly.
 *
 * The evidence (tools/graph_probe2.c churn_*): HIP 7.0
 * (70051831, the runtime torch 2.10+rocm7.0 bundles) crashes in
 * hipGraphLaunch once execs of graphs with parallel branches have been
 * destroyed -- a fork / join graph of two memsets, captured, launched and
 * destroyed in a loop, dies within 30 rounds, with no RCCL and no libmvx in
 * the process; kept alive, or without the fork, it never dies.  HIP 7.2
 * (70226015) runs all of it clean.  Round 4 met this as a SIGSEGV in the
 * launch of a graph captured after another was destroyed (p = 2 and 4 over
 * RCCL's socket transport).
 *
 * Knobs of a communicator, read at its creation (mvxi_graph_knobs):
 * MVX_GRAPH = 1 graphs on; MVX_GRAPH_CACHE = n (<= 32) the graphs it holds;
 * MVX_GRAPH_EVICT = 0 | 1 | 2 destroy mid-life none / single-branch / all;
 * MVX_GRAPH_FORK = 0 PIPE (whose capture forks to the combine stream and
 * joins back) stays eager.  Process-wide, read lazily (graph_destroy has no
 * communicator in hand): MVX_GRAPH_TRACE = 1, each capture step on stderr.
 */
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mvx_internal.h"

enum { G_FREE, G_SEEN, G_LIVE, G_RETIRED };     /* graph_ent_t.state */

__thread int mvxi_capturing;

void mvxi_gtrace(const char *what, int v)
{
    static int on = -1;
    const char *e;
    if (on < 0) on = (e = getenv("MVX_GRAPH_TRACE")) && atoi(e) == 1;
    if (on) fprintf(stderr, "mvx graph: %s %d\n", what, v);
}

/* ---- knobs and the public calls ------------------------------------------ */
/* the knob's value if set and within [lo, hi], else dflt */
static int knob(const char *name, int lo, int hi, int dflt)
{
    const char *e = getenv(name);
    const int v = e ? atoi(e) : dflt;
    return e && v >= lo && v <= hi ? v : dflt;
}

void mvxi_graph_knobs(mvx_comm_t *c)
{
    int v = 0, evict = MVX_GRAPH_EVICT_SERIAL;  /* what this runtime allows: all from HIP 7.2 on */
    if (hipRuntimeGetVersion(&v) != hipSuccess) (void)hipGetLastError();
    else if (v >= 70200000) evict = MVX_GRAPH_EVICT_ALL;
    c->graphs = knob("MVX_GRAPH", 1, 1, 0);
    c->graph_cap = knob("MVX_GRAPH_CACHE", 1, GRAPH_CACHE, GRAPH_CACHE);
    c->graph_evict = knob("MVX_GRAPH_EVICT", MVX_GRAPH_EVICT_NONE, MVX_GRAPH_EVICT_ALL, evict);
    c->graph_fork = knob("MVX_GRAPH_FORK", INT_MIN, INT_MAX, 1) != 0;
}

int mvx_comm_set_graphs(MPI_Comm comm, int on)
{
    mvx_comm_t *c = mvxi_get_comm(comm);
    if (!c) return ERR_COMM_NULL_CODE;
    /* turning graphs off keeps what was captured (destroyed with the
     * communicator); on again, they replay */
    c->graphs = on ? 1 : 0;
    c->graph_error = 0;
    return MPI_SUCCESS;
}

int mvx_comm_last_graph(MPI_Comm comm, int *state, int *error)
{
    mvx_comm_t *c = mvxi_get_comm(comm);
    if (!c) return ERR_COMM_NULL_CODE;
    if (state) *state = c->last_graph;
    if (error) *error = c->graph_error;
    return MPI_SUCCESS;
}

int mvx_comm_graph_stats(MPI_Comm comm, int *live, int *retired, long *destroyed)
{
    mvx_comm_t *c = mvxi_get_comm(comm);
    int i, l = 0, r = 0;
    if (!c) return ERR_COMM_NULL_CODE;
    for (i = 0; c->w && i < GRAPH_CACHE; i++) {
        l += c->w->graphs[i].state == G_LIVE;
        r += c->w->graphs[i].state == G_RETIRED;
    }
    if (live) *live = l;
    if (retired) *retired = r;
    if (destroyed) *destroyed = c->w ? c->w->graphs_destroyed : 0;
    return MPI_SUCCESS;
}

/* ---- the key --------------------------------------------------------------
 * Everything the captured work depends on, filled here and nowhere else
 * (zeroed first, so padding compares equal). */
static void graph_key(const mvx_comm_t *c, const job_t *J, hipStream_t st, graph_key_t *k)
{
    memset(k, 0, sizeof *k);
    memcpy(&k->plan, &J->P[0], sizeof k->plan);
    k->send = J->send[0]; k->recv = J->recv[0]; k->st = st; k->pool = c->pool;
    k->exch = c->exch; k->slices = c->exch_slices; k->keep = c->keep;
}

static unsigned long long graph_hash(const graph_key_t *k)
{
    const unsigned char *b = (const unsigned char *)k;
    unsigned long long h = 1469598103934665603ull;
    size_t i;
    for (i = 0; i < sizeof *k; i++) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

static int graph_match(const graph_ent_t *g, const graph_key_t *k, unsigned long long h)
{
    return (g->state == G_SEEN || g->state == G_LIVE) && g->hash == h && !memcmp(&g->key, k, sizeof *k);
}

/* ---- destruction ---------------------------------------------------------- */
static void graph_destroy(graph_ent_t *g)
{
    if ((g->state == G_LIVE || g->state == G_RETIRED) && g->exec) {
        mvxi_gtrace("destroy graph of variant", g->key.exch);
        hipGraphExecDestroy(g->exec);
    }
    if (g->done) hipEventDestroy(g->done);
    memset(g, 0, sizeof *g);
}

/* a graph destroyed mid-life, after its own last launch completed (its done
 * event), so none of it is in flight; counted for mvx_comm_graph_stats */
static void graph_evict(mvx_comm_t *c, graph_ent_t *g)
{
    if (g->done && hipEventSynchronize(g->done) != hipSuccess) (void)hipGetLastError();
    graph_destroy(g);
    c->w->graphs_destroyed++;
}

void mvxi_graphs_clear(mvx_comm_t *c)
{
    int i;
    if (!c->w) return;
    for (i = 0; i < GRAPH_CACHE; i++) {
        graph_destroy(&c->w->graphs[i]);
        memset(&c->w->seen[i], 0, sizeof c->w->seen[i]);
    }
}

/* may this graph's exec be destroyed now? */
static int graph_evictable(const mvx_comm_t *c, const graph_ent_t *g)
{
    if (c->graph_evict == MVX_GRAPH_EVICT_ALL) return 1;
    return c->graph_evict == MVX_GRAPH_EVICT_SERIAL && !g->forked;
}

/* The pool is about to be freed: every graph captured on it goes first --
 * destroyed where the runtime allows it, else retired. */
void mvxi_graphs_unpool(mvx_comm_t *c)
{
    int i, gone = 0;
    for (i = 0; i < GRAPH_CACHE; i++) {
        graph_ent_t *g = &c->w->graphs[i];
        if (c->w->seen[i].key.pool == c->pool) memset(&c->w->seen[i], 0, sizeof c->w->seen[i]);
        if (g->key.pool != c->pool) continue;
        if (g->state == G_LIVE) { g->state = G_RETIRED; gone += graph_evictable(c, g); }
    }
    for (i = 0; gone && i < GRAPH_CACHE; i++) {
        graph_ent_t *g = &c->w->graphs[i];
        if (g->state == G_RETIRED && graph_evictable(c, g)) graph_evict(c, g);
    }
}

/* ---- capture and launch --------------------------------------------------- */
/* 1 if the graph has parallel branches: a node with two or more successors,
 * or two or more roots (what HIP runs on parallel streams) */
static int graph_forked(hipGraph_t g)
{
    size_t ne = 0, nr = 0, i, j;
    hipGraphNode_t *from, *to;
    int forked = 0;
    if (hipGraphGetRootNodes(g, NULL, &nr) != hipSuccess || hipGraphGetEdges(g, NULL, NULL, &ne) != hipSuccess) {
        (void)hipGetLastError();
        return 1;                                   /* unknown: treat as forked */
    }
    if (nr > 1) return 1;
    if (!ne) return 0;
    from = (hipGraphNode_t *)malloc(ne * sizeof *from);
    to = (hipGraphNode_t *)malloc(ne * sizeof *to);
    if (!from || !to || hipGraphGetEdges(g, from, to, &ne) != hipSuccess) {
        (void)hipGetLastError();
        free(from);
        free(to);
        return 1;
    }
    for (i = 0; i < ne && !forked; i++)             /* out-degree >= 2 */
        for (j = i + 1; j < ne && !forked; j++) forked = from[i] == from[j];
    free(from);
    free(to);
    return forked;
}

static int graph_eligible(const mvx_comm_t *c, const job_t *J)
{
    return c->graphs && !c->graph_error && J->nr == 1 && !c->local && !c->has_ops && c->nccl && !c->timing &&
           J->P[0].opkind == MVX_OPKIND_PREDEFINED && !J->P[0].packed &&
           (c->exch != MVX_EXCH_PIPE || c->graph_fork);
}

/* launch g's exec on `st` (the null stream: forked onto the graph stream and
 * joined back) and record g->done where it ran */
static int graph_launch(mvx_comm_t *c, graph_ent_t *g, hipStream_t st)
{
    hipStream_t on = st ? st : c->gstream;
    if (st) {
        mvxi_gtrace("launch on the caller's stream", 0);
        if (hipGraphLaunch(g->exec, st) != hipSuccess) return MPI_ERR_OTHER;
    } else {
        mvxi_gtrace("launch: fork from the null stream", 0);
        if (mvxi_null_fork(c)) return MPI_ERR_OTHER;
        mvxi_gtrace("launch: hipGraphLaunch on the graph stream", 0);
        if (hipGraphLaunch(g->exec, c->gstream) != hipSuccess) return MPI_ERR_OTHER;
        mvxi_gtrace("launch: join to the null stream", 0);
        if (mvxi_null_join(c)) return MPI_ERR_OTHER;
    }
    return hipEventRecord(g->done, on) == hipSuccess ? MPI_SUCCESS : MPI_ERR_OTHER;
}

/* capture the job on `cs` into an executable graph (nothing runs) */
static int graph_capture(mvx_comm_t *c, const job_t *J, hipStream_t cs, hipGraphExec_t *out, int *forked)
{
    hipGraph_t g = NULL;
    hipError_t e;
    int rc;
    *out = NULL;
    mvxi_gtrace("begin capture, variant", c->exch);
    if (hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        (void)hipGetLastError();
        return MPI_ERR_OTHER;
    }
    mvxi_capturing = 1;
    rc = mvxi_run_device_eager(c, J, cs);
    mvxi_capturing = 0;
    mvxi_gtrace("captured job, rc", rc);
    e = hipStreamEndCapture(cs, &g);
    mvxi_gtrace("end capture, hip error", (int)e);
    if (rc || e != hipSuccess || !g) {
        if (g) hipGraphDestroy(g);
        (void)hipGetLastError();
        return rc ? rc : MPI_ERR_OTHER;
    }
    *forked = graph_forked(g);
    e = hipGraphInstantiate(out, g, NULL, NULL, 0);
    mvxi_gtrace("instantiate, hip error", (int)e);
    mvxi_gtrace("instantiated graph has parallel branches", *forked);
    hipGraphDestroy(g);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        *out = NULL;
        return MPI_ERR_OTHER;
    }
    return MPI_SUCCESS;
}

static int run_uncaptured(mvx_comm_t *c, const job_t *J, hipStream_t st)
{
    c->last_graph = 0;
    return mvxi_run_device_eager(c, J, st);
}

/* Graph slots hold captured graphs only; jobs seen once wait in a table of
 * their own (mvx_work.seen, least recently seen replaced).  A job runs
 * eagerly at its first sighting and is captured at its second: only then,
 * when every slot holds a graph, is the least recently used evictable one
 * destroyed.  A communicator with more distinct jobs than slots thus keeps
 * its graphs instead of trading one for every new job it sees. */
static int run_device_graph(mvx_comm_t *c, const job_t *J, hipStream_t st)
{
    mvx_work *w = mvxi_work(c);
    graph_ent_t *g = NULL, *slot = NULL, *seen = NULL, *sslot = NULL, *lru = NULL;
    graph_key_t k;
    unsigned long long h;
    int i, rc, forked = 1;
    if (!w || (!st && mvxi_graph_streams(c))) return mvxi_run_device_eager(c, J, st);
    graph_key(c, J, st, &k);
    h = graph_hash(&k);
    for (i = 0; i < c->graph_cap; i++) {
        graph_ent_t *e = &w->graphs[i];
        if (graph_match(e, &k, h)) { g = e; break; }
        if (e->state == G_FREE && !slot) slot = e;
        if (e->state == G_LIVE && graph_evictable(c, e) && (!lru || e->stamp < lru->stamp)) lru = e;
    }
    if (g) {                                                   /* replay */
        g->stamp = ++w->graph_clock;
        c->ran_exch = g->ran_exch;
        c->last_graph = 1;
        return graph_launch(c, g, st);
    }
    for (i = 0; i < GRAPH_CACHE; i++) {
        graph_ent_t *e = &w->seen[i];
        if (graph_match(e, &k, h)) { seen = e; break; }
        if (!sslot || (sslot->state != G_FREE && (e->state == G_FREE || e->stamp < sslot->stamp))) sslot = e;
    }
    if (!seen) {                                               /* first sighting: eager */
        if ((rc = run_uncaptured(c, J, st))) return rc;
        graph_key(c, J, st, &k);                               /* the pool as the call left it */
        memset(sslot, 0, sizeof *sslot);
        sslot->state = G_SEEN;
        sslot->key = k;
        sslot->hash = graph_hash(&k);
        sslot->stamp = ++w->graph_clock;
        return MPI_SUCCESS;
    }
    /* second sighting: capture, into a free slot or the LRU graph's */
    if (!slot && lru) {
        graph_evict(c, lru);
        slot = lru;
    }
    memset(seen, 0, sizeof *seen);
    if (!slot) return run_uncaptured(c, J, st);                /* every slot holds a graph it may not destroy */
    if (hipEventCreateWithFlags(&slot->done, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        slot->done = NULL;
        return run_uncaptured(c, J, st);
    }
    rc = graph_capture(c, J, st ? st : c->gstream, &slot->exec, &forked);
    if (rc) {
        c->graph_error = rc;
        graph_destroy(slot);
        return run_uncaptured(c, J, st);
    }
    slot->state = G_LIVE;                                      /* a capture grows no pool: k still holds */
    slot->key = k;
    slot->hash = h;
    slot->forked = forked;
    slot->ran_exch = c->ran_exch;
    slot->stamp = ++w->graph_clock;
    c->last_graph = 2;
    rc = graph_launch(c, slot, st);
    mvxi_gtrace("first launch, rc", rc);
    return rc;
}

int mvxi_run_device(mvx_comm_t *c, const job_t *J, hipStream_t st)
{
    if (graph_eligible(c, J)) return run_device_graph(c, J, st);
    return run_uncaptured(c, J, st);
}
