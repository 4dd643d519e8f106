// The body of a kernel that walks caller rays on the 8-wide BVH, included INSIDE the kernel (query_walk.h says where and why text, not a template):
// the decoupled walk of the wavefront kernels (pt_wavefront.h: traceClosestWideBody).  Per turn a lane tests at most one pending record and visits at
// most one node; a lane whose walk is over stores its answer and is idle; the wave claims once `refillAt` of its lanes are.  A lane's walk is a pure
// function of its ray -- records are tested in the order traverseClosestWide tests them, and a node visited before an earlier node's records have
// shortened the ray only reports children that begin behind the hit --, so the closest hit is traverseClosestWide's whatever the turn order.
// (No hoisted quad here: the record order is the sequential walk's.)
// The kernel has `DeviceScene s`, `uint32_t n`, `uint32_t *counter` (query_walk.h: claimRays) and `uint32_t refillAt` in scope and defines
//   QUERY_WALK_OCCLUDED                  a constant; true: the same loop, ended at the first accepted record, the ray's tmax never shortened
//   QUERY_WALK_LOAD(j, index)            an expression: the RayD at place j of the batch, `index` set to where its answer goes
//   QUERY_WALK_STORE(index, hit, found)  a statement: the answer of a finished walk
    extern __shared__ int ldsStack[];
    uint2 *stack = reinterpret_cast<uint2 *>(ldsStack) + threadIdx.x;
    const int stride = RAY_QUERY_THREADS;
    bool busy = false, exhausted = false;
    uint32_t index = 0;
    RayD ray; ray.o = splat3(0.0f); ray.d = splat3(1.0f); ray.tmin = 0.0f; ray.tmax = 0.0f;
    WideRay wr; wr.idir = splat3(1.0f); wr.octInv = 0u;
    WideState w;
    wideStart(w);
    float tmax = 0.0f;
    float4 hit = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
    for (;;) {
        unsigned long long busyMask = __ballot(busy);
        if (!exhausted && 64u - (uint32_t)__popcll(busyMask) >= refillAt) {
            const uint32_t j = claimRays(counter, !busy, n, exhausted);
            if (!busy && j < n) {
                ray = QUERY_WALK_LOAD(j, index);
                wr = wideRaySetup(ray);
                wideStart(w);
                tmax = ray.tmax;
                hit = make_float4(tmax, 0.0f, 0.0f, __int_as_float(-1));
                busy = true;
            }
            busyMask = __ballot(busy);
        }
        if (busyMask == 0ull)
            break;                               // (an idle wave has claimed above, refillAt <= 64: the counter has passed n)
        uint32_t recIdx = 0, nodeIdx = 0;
        bool hasRec = false, hasNode = false;
        if (busy) {
            if (w.triMask == 0u && w.tri2Mask != 0u) { w.triBase = w.tri2Base; w.triMask = w.tri2Mask; w.triValid = w.tri2Valid; w.tri2Mask = 0u; }
            if (w.triMask) {
                const uint32_t b = (uint32_t)__ffs((int)w.triMask) - 1u;
                recIdx = w.triBase + (uint32_t)__popc(w.triValid & ((1u << b) - 1u));
                w.triMask &= w.triMask - 1u;
                hasRec = true;
            }
            if (w.tri2Mask == 0u)                // (room for the records of the node visited now)
                hasNode = wideNextNode(w, wr.octInv, stack, stride, nodeIdx);
        }
        float4 r0, r1, r2;
        WideNodeRegs nd;
        PT_WALK_FETCH(s, r0, r1, r2, nd, hasRec, recIdx, hasNode, nodeIdx);
        bool found = false;
        if (hasRec) {
            uint32_t meta;
            if (QUERY_WALK_OCCLUDED) {
                float t = ray.tmax;
                found = testRecordLoaded<false, KINDS_ALL>(s, recIdx, r0, r1, r2, ray, t, hit, meta);
            } else {
                (void)testRecordLoaded<false, KINDS_ALL>(s, recIdx, r0, r1, r2, ray, tmax, hit, meta);
            }
        }
        if (hasNode) {
            const uint32_t ob = w.triBase, om = w.triMask, ov = w.triValid;
            wideVisit(w, nd, ray.o, wr, ray.tmin, QUERY_WALK_OCCLUDED ? ray.tmax : tmax);
            if (om) { w.tri2Base = w.triBase; w.tri2Mask = w.triMask; w.tri2Valid = w.triValid; w.triBase = ob; w.triMask = om; w.triValid = ov; }
        }
        if (busy && (found || wideWalkOver(w))) {    // (in the turn that looked at the walk's last record / node)
            QUERY_WALK_STORE(index, hit, found);
            busy = false;
        }
    }
#undef QUERY_WALK_OCCLUDED
#undef QUERY_WALK_LOAD
#undef QUERY_WALK_STORE
