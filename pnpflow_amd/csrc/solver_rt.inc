// solver_rt.inc -- what every solver on the engine shares on the host side: the device buffers of a solver state (DevBufs), a cached hipGraph
// (CachedGraph) and the stream a graph can be captured on (graph_stream).  Included in engine.hip before build_plan and the solvers.

// An owning set of device buffers.  The state structs keep their named pointers; the set remembers what it handed out, so a state is freed
// with release() followed by *st = State{}, and pf_engine_memory_bytes counts exactly the bytes that were asked for.
struct DevBufs {
    std::vector<void*> ptrs;
    int64_t bytes = 0;
    // one buffer of `nbytes` into *slot, poisoned under `group` (PNPFLOW_HIP_POISON); may be called on a set that already holds buffers
    template <class T>
    hipError_t try_alloc(pf_engine* e, T** slot, size_t nbytes, int group) {
        void* p = nullptr;
        const hipError_t r = hipMalloc(&p, nbytes);
        if (r != hipSuccess) return r;
        poison(p, nbytes, group);
        ptrs.push_back(p); bytes += (int64_t)nbytes; e->bytes += (int64_t)nbytes;
        *slot = (T*)p;
        return hipSuccess;
    }
    template <class T>
    int alloc(pf_engine* e, T** slot, size_t nbytes, int group) {
        const hipError_t r = try_alloc(e, slot, nbytes, group);
        if (r != hipSuccess) { e->err = std::string("hipMalloc of ") + std::to_string(nbytes) + " bytes of solver state: " + hipGetErrorString(r); return PF_ERR_HIP; }
        return PF_OK;
    }
    // `count` 4-byte elements, at least 64 of them (the small tables and counters are read in whole wavefronts), poison group 4
    template <class T>
    int alloc4(pf_engine* e, T** slot, size_t count) { return alloc(e, slot, std::max<size_t>(count, 64) * 4, 4); }
    void release(pf_engine* e) {
        for (void* p : ptrs) hipFree(p);
        e->bytes -= bytes;
        ptrs.clear(); bytes = 0;
    }
};

// A captured sequence of launches, kept while the arguments baked into it (the key, compared bytewise: plain structs without padding, zeroed
// before they are filled) stay the same.  A live graph is listed in e->graphs, which is all that drop_all_graphs (precision mode, solver time
// scale, teardown) and plan_is_held (the plan cache's eviction) look at: a solver that captures through this type cannot be missed by either.
struct CachedGraph {
    hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
    std::vector<unsigned char> key;
    std::vector<const void*> plans;         // the plans whose launches (and activation buffers) the nodes replay
    bool live() const { return exec != nullptr; }
    void drop(pf_engine* e) {
        if (exec) hipGraphExecDestroy(exec);
        if (graph) hipGraphDestroy(graph);
        e->graphs.erase(std::remove(e->graphs.begin(), e->graphs.end(), this), e->graphs.end());
        *this = CachedGraph{};
    }
    // drops a graph captured under another key; true if a graph for `k` is cached afterwards
    template <class K>
    bool keep_for(pf_engine* e, const K& k) {
        if (exec && (key.size() != sizeof k || memcmp(key.data(), &k, sizeof k) != 0)) drop(e);
        return live();
    }
    // captures what enqueue() puts on s (nothing runs); `held`: the plans enqueue() launches
    template <class K, class F>
    int capture(pf_engine* e, hipStream_t s, const K& k, std::initializer_list<const void*> held, F&& enqueue) {
        drop(e);
        HIPCHK(e, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        const int rc = enqueue();
        hipGraph_t g = nullptr;
        const hipError_t ce = hipStreamEndCapture(s, &g);
        if (rc != PF_OK) { if (g) hipGraphDestroy(g); return rc; }
        if (ce != hipSuccess) { e->err = std::string("hipStreamEndCapture: ") + hipGetErrorString(ce); return PF_ERR_HIP; }
        hipGraphExec_t x = nullptr;
        const hipError_t ie = hipGraphInstantiate(&x, g, nullptr, nullptr, 0);
        if (ie != hipSuccess) { hipGraphDestroy(g); e->err = std::string("hipGraphInstantiate: ") + hipGetErrorString(ie); return PF_ERR_HIP; }
        graph = g; exec = x; plans.assign(held);
        key.assign((const unsigned char*)&k, (const unsigned char*)&k + sizeof k);
        e->graphs.push_back(this);
        return PF_OK;
    }
    int launch(pf_engine* e, hipStream_t s) { HIPCHK(e, hipGraphLaunch(exec, s)); return PF_OK; }
};

static void drop_all_graphs(pf_engine* e) { while (!e->graphs.empty()) e->graphs.back()->drop(e); }

static bool plan_is_held(const pf_engine* e, const void* plan) {
    for (const CachedGraph* g : e->graphs)
        if (std::find(g->plans.begin(), g->plans.end(), plan) != g->plans.end()) return true;
    return false;
}

// The stream a solver call runs on.  The legacy NULL stream cannot be captured: when a graph is wanted (`need`) the call runs on an
// engine-owned stream instead, ordered after everything already enqueued on the NULL stream (the solver calls synchronise before returning).
// The stream is a BLOCKING one (hipStreamDefault): work a callback puts on the NULL stream and the engine's next launches stay ordered by the
// legacy-stream rule (round 2: on a non-blocking stream, metric kernels launched from the callbacks on the NULL stream and cached-graph replays
// produced NaNs on the second batch; the Python solvers also hand over a real stream)
static int graph_stream(pf_engine* e, bool need, hipStream_t& s) {
    if (!need || s != nullptr) return PF_OK;
    if (!e->work_stream) HIPCHK(e, hipStreamCreateWithFlags(&e->work_stream, hipStreamDefault));
    HIPCHK(e, hipStreamSynchronize(nullptr));
    s = e->work_stream;
    return PF_OK;
}

// the operator rules (deg_rules.h) every solver applies to its H x H images before it allocates, copies or launches anything (`who`: the prefix of the
// message); Hy: the side of the measurement
static int check_operator(pf_engine* e, const char* who, const pf_degradation* d, int H, int& Hy) {
    const DegView dv = to_view(d);
    if (const char* broken = deg_rule_violation(dv, H, H)) { e->err = std::string(who) + ": " + broken; return PF_ERR_INVALID; }
    Hy = deg_out_side(dv, H);
    return PF_OK;
}

// frees a heap-held solver state the way a shape change does (State::reset), then the struct itself
template <class S>
static void free_state(pf_engine* e, S*& st) {
    if (!st) return;
    st->reset(e);
    delete st;
    st = nullptr;
}
