// CPU check of what the learners' train calls share on the host behind their plans
// (dronerl_amd/csrc/dronerl_learn_args.h and per/dronerl_per_learn_args.h: plain C++, no HIP call).  For each net
// family -- dense 8-8 at batches 1 and 4096 (also as the prioritized chain's block), the wide family's 256-wide
// limit, the smallest conv description of the conv layout checks at the small and the large learner's plan -- and
// for the uniform and the prioritized order:
//   * every fault of one list (the hyperparameters' ranges, NULL and misaligned blocks, the ring's members, its
//     capacity and the size, short, f32-for-code and misaligned rows, the PER hyperparameters and block) is refused
//     with its text, the same text in every family but for the two differences the table names: the conv nets'
//     name for short rows, and the prioritized calls' capacity refusal, which is the tree's plan's;
//   * a refused call leaves the argument block, the drawn rows, the tree's view and the sampler's untouched;
//   * a good call puts every pointer at the fake base + the public layout's offset and every hyperparameter in.
// Stand-alone host code, built and run by tests/test_large_batch_learner.py under the address and
// undefined-behaviour sanitizers.  (tests/test_learner_refusals.py asks the library's calls themselves.)
#include <stdio.h>
#include <string.h>

#include <functional>
#include <vector>

#include "../../dronerl_amd/csrc/convlarge/dronerl_convlarge_layout.h"
#include "../../dronerl_amd/csrc/dronerl_learn_args.h"
#include "../../dronerl_amd/csrc/largelearn/dronerl_largelearn_layout.h"
#include "../../dronerl_amd/csrc/per/dronerl_per_learn_args.h"
#include "../../dronerl_amd/csrc/widenet/dronerl_widenet_layout.h"

static int bad = 0;

#define EXPECT(cond)                                              \
    do {                                                          \
        if (!(cond)) {                                            \
            printf("  line %d: %s\n", __LINE__, #cond);           \
            ++bad;                                                \
        }                                                         \
    } while (0)

// fake device addresses: never dereferenced
static const uintptr_t kAgent = 0x10000000, kPacked = 0x20000000, kPer = 0x30000000, kRing = 0x40000000;

struct Call {
    drl_dqn_hparams h;
    drl_per_hparams ph;
    bool ph_null = false, r_null = false;
    uintptr_t agent = kAgent, packed = kPacked, per = kPer;
    drl_replay r;
    int64_t size = 100;
};

static Call good_call(int batch, int obs_floats) {
    Call c;
    c.h = drl_dqn_hparams{batch, 10, 5, 0, 0.9, 1e-3, 0.9, 0.999, 1e-8, 1.0, 0.99, 0.01, 1234};
    c.ph = drl_per_hparams{0.6, 0.4, 1000, 1e-6};
    c.r = drl_replay{5000,
                     obs_floats,
                     reinterpret_cast<float*>(kRing),
                     reinterpret_cast<float*>(kRing + 0x1000000),
                     reinterpret_cast<int32_t*>(kRing + 0x2000000),
                     reinterpret_cast<float*>(kRing + 0x3000000),
                     reinterpret_cast<uint8_t*>(kRing + 0x4000000)};
    return c;
}

enum Kind { kBoth, kPerOnly };

struct Fault {
    const char* name;
    Kind kind;
    const char* uniform_text;  // what the uniform order answers (kPerOnly: unused)
    const char* per_text;      // ... and the prioritized one; nullptr: the same
    std::function<void(Call&)> apply;
};

static const char* kCapacity = "replay capacity must be in [1, 2^31)";
static const char* kPerCapacity = "capacity must be in [1, 2^24] (DRL_PER_MAX_CAPACITY)";  // difference 2: per::plan's
static const char* kAgentText = "the agent block must be a 16-byte aligned device pointer";
static const char* kPackedText = "packed buffer must be a 16-byte aligned device pointer";
static const char* kPerBlock = "the prioritized replay block must be a 16-byte aligned device pointer";
static const char* kSHORT = "<the family's short-rows text>";  // difference 1: resolved per family

static std::vector<Fault> faults() {
    return {
        {"target_update_interval 0", kBoth, "target_update_interval and epsilon_decay_every must be >= 1", nullptr,
         [](Call& c) { c.h.target_update_interval = 0; }},
        {"epsilon_decay_every 0", kBoth, "target_update_interval and epsilon_decay_every must be >= 1", nullptr,
         [](Call& c) { c.h.epsilon_decay_every = 0; }},
        {"beta1 1.0", kBoth, "beta1 and beta2 must be in [0, 1)", nullptr, [](Call& c) { c.h.beta1 = 1.0; }},
        {"beta2 -0.1", kBoth, "beta1 and beta2 must be in [0, 1)", nullptr, [](Call& c) { c.h.beta2 = -0.1; }},
        {"agent NULL", kBoth, kAgentText, nullptr, [](Call& c) { c.agent = 0; }},
        {"agent misaligned", kBoth, kAgentText, nullptr, [](Call& c) { c.agent += 8; }},
        {"packed NULL", kBoth, kPackedText, nullptr, [](Call& c) { c.packed = 0; }},
        {"packed misaligned", kBoth, kPackedText, nullptr, [](Call& c) { c.packed += 4; }},
        {"r NULL", kBoth, "replay buffers are NULL", nullptr, [](Call& c) { c.r_null = true; }},
        {"r.obs NULL", kBoth, "replay buffers are NULL", nullptr, [](Call& c) { c.r.obs = nullptr; }},
        {"r.next_obs NULL", kBoth, "replay buffers are NULL", nullptr, [](Call& c) { c.r.next_obs = nullptr; }},
        {"r.actions NULL", kBoth, "replay buffers are NULL", nullptr, [](Call& c) { c.r.actions = nullptr; }},
        {"r.rewards NULL", kBoth, "replay buffers are NULL", nullptr, [](Call& c) { c.r.rewards = nullptr; }},
        {"r.dones NULL", kBoth, "replay buffers are NULL", nullptr, [](Call& c) { c.r.dones = nullptr; }},
        {"capacity 0", kBoth, kCapacity, kPerCapacity, [](Call& c) { c.r.capacity = 0; }},
        {"capacity 2^31", kBoth, kCapacity, kPerCapacity, [](Call& c) { c.r.capacity = (int64_t)1 << 31; }},
        {"size -1", kBoth, "size must be in [0, capacity]", nullptr, [](Call& c) { c.size = -1; }},
        {"size capacity+1", kBoth, "size must be in [0, capacity]", nullptr, [](Call& c) { c.size = c.r.capacity + 1; }},
        {"short rows", kBoth, kSHORT, nullptr, [](Call& c) { c.r.obs_floats -= 2; }},
        {"rows misaligned", kBoth, "replay rows must be 4-byte aligned", nullptr,
         [](Call& c) { c.r.obs = reinterpret_cast<float*>(kRing + 2); }},
        {"next rows misaligned", kBoth, "replay rows must be 4-byte aligned", nullptr,
         [](Call& c) { c.r.next_obs = reinterpret_cast<float*>(kRing + 0x1000001); }},
        {"ph NULL", kPerOnly, nullptr, "the prioritized replay's hparams are NULL", [](Call& c) { c.ph_null = true; }},
        {"alpha -1", kPerOnly, nullptr, "alpha must be >= 0", [](Call& c) { c.ph.alpha = -1.0; }},
        {"beta0 2", kPerOnly, nullptr, "beta0 must be in [0, 1]", [](Call& c) { c.ph.beta0 = 2.0; }},
        {"beta_steps -1", kPerOnly, nullptr, "beta_steps must be >= 0", [](Call& c) { c.ph.beta_steps = -1; }},
        {"per eps -1", kPerOnly, nullptr, "eps must be >= 0", [](Call& c) { c.ph.eps = -1.0; }},
        {"per NULL", kPerOnly, nullptr, kPerBlock, [](Call& c) { c.per = 0; }},
        {"per misaligned", kPerOnly, nullptr, kPerBlock, [](Call& c) { c.per += 8; }},
        {"capacity 2^24 + 1", kPerOnly, nullptr, kPerCapacity, [](Call& c) { c.r.capacity = (1 << 24) + 1; }},
    };
}

// everything a prioritized call writes besides the argument block
struct PerOut {
    drl::per::Drawn d;
    drl::per::TreeArgs t;
    drl::per::SampleArgs sa;
};

template <class A>
static const char* issue(bool prioritized, A& a, PerOut& o, int in_floats, const char* short_rows, const Call& c) {
    void* agent = reinterpret_cast<void*>(c.agent);
    void* packed = reinterpret_cast<void*>(c.packed);
    const drl_replay* r = c.r_null ? nullptr : &c.r;
    if (!prioritized) return drl::learn_args(a, in_floats, short_rows, &c.h, agent, packed, r, c.size);
    return drl::per::learn_args(a, o.d, in_floats, short_rows, &c.h, c.ph_null ? nullptr : &c.ph, agent, packed, r, c.size,
                                reinterpret_cast<void*>(c.per), &o.t, &o.sa);
}

template <class T>
static std::vector<uint8_t> bytes_of(const T& v) {
    const uint8_t* p = reinterpret_cast<const uint8_t*>(&v);
    return std::vector<uint8_t>(p, p + sizeof v);
}

static uintptr_t at(const void* p) { return reinterpret_cast<uintptr_t>(p); }

// `planned`: a zeroed argument block with its plan in; `coded`: the same net taking policy codes (or nullptr)
template <class A>
static void family(const char* name, const A& planned, const A* coded, int in_floats, const char* short_rows) {
    const int before = bad;
    const int batch = planned.P.batch;
    for (int prioritized = 0; prioritized < 2; ++prioritized) {
        // (heap: the sanitizer sees a write past the block)
        std::vector<A> holder(1, planned);
        std::vector<PerOut> oholder(1);
        A& a = holder[0];
        PerOut& o = oholder[0];
        memset(&o, 0x5A, sizeof o);
        const std::vector<uint8_t> a0 = bytes_of(a), o0 = bytes_of(o);
        for (const Fault& f : faults()) {
            if (f.kind == kPerOnly && !prioritized) continue;
            Call c = good_call(batch, in_floats);
            f.apply(c);
            const char* want = prioritized && f.per_text ? f.per_text : f.uniform_text;
            if (want == kSHORT) want = short_rows;
            const char* got = issue(prioritized, a, o, in_floats, short_rows, c);
            if (!got || strcmp(got, want)) {
                printf("  %s (%s) %s: got \"%s\", want \"%s\"\n", name, prioritized ? "prioritized" : "uniform", f.name,
                       got ? got : "(accepted)", want);
                ++bad;
            }
            EXPECT(bytes_of(a) == a0 && bytes_of(o) == o0);  // a refused call writes nothing
        }
        if (coded) {  // f32 rows for a code net
            std::vector<A> ch(1, *coded);
            const std::vector<uint8_t> c0 = bytes_of(ch[0]);
            const char* got = issue(prioritized, ch[0], o, in_floats, short_rows, good_call(batch, in_floats));
            EXPECT(got && strstr(got, "replay rows are policy codes"));
            EXPECT(bytes_of(ch[0]) == c0 && bytes_of(o) == o0);
        }
        // the good call
        const Call c = good_call(batch, in_floats);
        const char* got = issue(prioritized, a, o, in_floats, short_rows, c);
        EXPECT(got == nullptr);
        if (got) continue;
        const auto& u = a.P.pub;
        EXPECT(at(a.online) == kAgent + u.online_off && at(a.target) == kAgent + u.target_off);
        EXPECT(at(a.adam_m) == kAgent + u.m_off && at(a.adam_v) == kAgent + u.v_off);
        EXPECT(at(a.ctr) == kAgent + u.counters_off && at(a.scratch) == kAgent + u.scratch_off);
        EXPECT(u.online_off < u.target_off && u.target_off < u.m_off && u.m_off < u.v_off &&
               u.v_off < u.counters_off && u.counters_off < u.scratch_off && u.scratch_off < u.bytes);
        EXPECT(at(a.r_obs) == at(c.r.obs) && at(a.r_next) == at(c.r.next_obs) && at(a.r_act) == at(c.r.actions) &&
               at(a.r_rew) == at(c.r.rewards) && at(a.r_done) == at(c.r.dones));
        EXPECT(a.pack_status == nullptr);  // (the pack's to set)
        EXPECT(a.row_words == c.r.obs_floats && a.size == c.size && a.seed == c.h.sample_seed);
        EXPECT(a.trained == (c.size >= batch) && a.code_w == a.P.code_w);
        EXPECT(a.gamma == (float)c.h.gamma && a.b1 == (float)c.h.beta1 && a.b2 == (float)c.h.beta2);
        EXPECT(a.c1 == (float)(1.0 - c.h.beta1) && a.c2 == (float)(1.0 - c.h.beta2) && a.adam_eps == (float)c.h.adam_eps);
        EXPECT(a.neg_lr == (float)(-c.h.learning_rate) && a.tau == (float)c.h.tau &&
               a.one_minus_tau == (float)(1.0 - c.h.tau));
        EXPECT(a.eps_decay == (float)c.h.epsilon_decay && a.eps_end == (float)c.h.epsilon_end);
        EXPECT(a.b1d == c.h.beta1 && a.b2d == c.h.beta2 && a.target_every == c.h.target_update_interval &&
               a.eps_every == c.h.epsilon_decay_every);
        EXPECT(bytes_of(a.P) == bytes_of(planned.P));  // the plan is the caller's
        if (!prioritized) {
            EXPECT(bytes_of(o) == o0);
            continue;
        }
        drl::per::Plan T;
        EXPECT(drl::per::plan(c.r.capacity, batch, &T) == nullptr);
        const drl_per_layout& v = T.pub;
        EXPECT(at(o.t.tree) == kPer + v.tree_off && at(o.t.pmax) == kPer + v.pmax_off && at(o.t.wmax) == kPer + v.wmax_off);
        EXPECT(at(o.t.slots) == kPer + v.slots_off && at(o.t.weights) == kPer + v.weights_off &&
               at(o.t.absd) == kPer + v.absd_off);
        EXPECT(o.t.capacity == c.r.capacity && o.t.P == v.leaves && o.t.batch == batch);
        EXPECT(at(o.d.slots) == at(o.t.slots) && at(o.d.weights) == at(o.t.weights) && at(o.d.absd) == at(o.t.absd));
        EXPECT(at(o.d.leaves) == at(o.t.tree) + 4 * (uintptr_t)o.t.P && at(o.d.pmax) == at(o.t.pmax));
        EXPECT(o.d.alpha == c.ph.alpha && o.d.per_eps == c.ph.eps);
        EXPECT(o.sa.seed == c.h.sample_seed && o.sa.size == c.size && o.sa.beta0 == c.ph.beta0 &&
               o.sa.beta_steps == c.ph.beta_steps);
    }
    printf("%s: %s\n", name, bad == before ? "ok" : "FAILED");
}

static drl::ll::LearnArgs dense(std::vector<int32_t> sizes, int code_w, int batch, int max_width = drl::ll::kMaxWidth) {
    drl::ll::LearnArgs a;
    memset(&a, 0, sizeof a);
    const char* msg = drl::ll::plan((int)sizes.size() - 1, sizes.data(), sizes.data() + 1, code_w, batch, &a.P, max_width);
    if (msg) printf("  dense plan refused: %s\n", msg);
    bad += msg != nullptr;
    return a;
}

static drl::ll::LearnArgs wide(int input, int batch) {
    drl_widenet_desc d;
    memset(&d, 0, sizeof d);
    d.in_features = 294;
    d.n_hidden = 3;
    d.hidden[0] = drl::wn::kMaxWidth;
    d.hidden[1] = 128;
    d.hidden[2] = 64;
    d.n_actions = 5;
    d.input = input;
    drl::wn::Layout L;
    const char* msg = drl::wn::layout(&d, &L);
    if (msg) printf("  wide layout refused: %s\n", msg);
    bad += msg != nullptr;
    std::vector<int32_t> sizes;
    for (int l = 0; l < L.n_layers; ++l) sizes.push_back(L.l[l].in);
    sizes.push_back(L.l[L.n_layers - 1].out);
    return dense(sizes, L.code_w, batch, drl::wn::kMaxWidth);
}

static drl_convnet_desc conv_desc(int W, int co, int k, int s, int p, int dense0, int input) {
    drl_convnet_desc d;
    memset(&d, 0, sizeof d);
    d.window = W;
    d.n_conv = 1;
    d.conv[0] = {co, k, s, p};
    d.n_dense = 1;
    d.dense[0] = dense0;
    d.n_actions = 5;
    d.input = input;
    return d;
}

static drl::cl::LearnArgs conv(const drl_convnet_desc& d, int batch, bool large) {
    drl::cl::LearnArgs a;
    memset(&a, 0, sizeof a);
    const char* msg;
    if (large) {
        drl::cg::Plan P;
        msg = drl::cg::plan(&d, batch, &P);
        a.P = P.c;
    } else {
        msg = drl::cl::plan(&d, batch, &a.P);
    }
    if (msg) printf("  conv plan refused: %s\n", msg);
    bad += msg != nullptr;
    return a;
}

int main() {
    // dense 8-8 on a 5x5 window (150 inputs: the smallest a policy-code twin exists for) at both ends of the batch range
    for (int batch : {1, 4096}) {
        const drl::ll::LearnArgs d = dense({150, 8, 8, 5}, 0, batch), dc = dense({150, 8, 8, 5}, 5, batch);
        family(batch == 1 ? "dense 150-8-8-5 @1" : "dense 150-8-8-5 @4096", d, &dc, 150, drl::kShortRowsDense);
        // ... and as the prioritized chain's block, which derives from it
        drl::per::LearnArgs p, pc;
        memset(&p, 0, sizeof p);
        memset(&pc, 0, sizeof pc);
        p.P = d.P;
        pc.P = dc.P;
        family(batch == 1 ? "dense (per block) @1" : "dense (per block) @4096", p, &pc, 150, drl::kShortRowsDense);
    }
    {
        const drl::ll::LearnArgs w = wide(DRL_QNET_INPUT_OBS, 256), wc = wide(DRL_QNET_INPUT_CODE, 256);
        family("wide 294-256-128-64-5 @256", w, &wc, 294, drl::kShortRowsDense);
    }
    {
        // convlearn_layout_check's smallest net (a 3x3 window, one 1x1 conv layer, f32 rows only) ...
        const drl_convnet_desc e = conv_desc(3, 32, 1, 1, 0, 8, DRL_QNET_INPUT_OBS);
        const drl::cl::LearnArgs s = conv(e, 8, false), g = conv(e, 4096, true);
        family<drl::cl::LearnArgs>("conv 3x3 @8", s, nullptr, s.P.in, drl::kShortRowsConv);
        family<drl::cl::LearnArgs>("conv 3x3 @4096 (large plan)", g, nullptr, g.P.in, drl::kShortRowsConv);
        // ... and its smallest with a policy-code twin (7x7, the reference's dqn-agent-5 shape)
        const drl_convnet_desc a7 = conv_desc(7, 4, 3, 1, 1, 8, DRL_QNET_INPUT_OBS),
                               c7 = conv_desc(7, 4, 3, 1, 1, 8, DRL_QNET_INPUT_CODE);
        const drl::cl::LearnArgs a = conv(a7, 64, false), ac = conv(c7, 64, false);
        family("conv 7x7 @64", a, &ac, a.P.in, drl::kShortRowsConv);
    }
    printf(bad ? "FAILED: %d\n" : "OK\n", bad);
    return bad ? 1 : 0;
}
