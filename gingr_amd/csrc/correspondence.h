// The correspondence flavour of the fitter -- CPD, ICP on the point cloud, ICP on the surface, pairs given by the caller -- as ONE
// descriptor: the C ABI's (flavour, cpd params, icp params) triple is turned into a Correspondence once per ABI call and every phase
// function, exchange driver and query of the fitter family takes it by reference.  Everything that follows from the flavour is a
// function here; nothing else compares flavour integers.  Plain C++ for the host, no HIP and no fitter types: the library includes it
// through gp.h and tests/c/correspondence_driver.cpp tabulates it under the sanitizers.
//
// Order of the precondition checks of an entry point that takes a flavour (fitter.hip: check_correspondence does the middle three):
//   1 handle          the fitter / group pointer is null                                   -> GINGR_ERR_BAD_ARGUMENT, no text
//   2 ready           target and state set (check_ready)                                   -> GINGR_ERR_STATE
//   3 parameters      the rules of correspondence_error below                              -> GINGR_ERR_BAD_ARGUMENT
//   4 flavour         meshes set for the surface flavour; the planes of the pairs flavour  -> GINGR_ERR_STATE
//   5 the operation's own (null results, single shard only, one iteration per sampled proposal ...)
// Entry points that take the flavour as an integer refuse one outside their own range with their own answer between 2 and 3 (the
// fitter's: "... bad arguments" / "mh_step: bad request") or together with 1 (the group's, which has no text for it).
// gingr_fitter_mh_step measures its likelihood on the surfaces whatever the flavour: it asks for the meshes itself, with its own text.
#pragma once
#include <cstdint>

#include "../../include/gingr_hip.h"

enum class Flavour : int32_t { Cpd = 0, IcpCloud = 1, IcpSurface = 2, Pairs = 3 };  // the ABI's integers

struct Correspondence {
    Flavour kind;
    gingr_cpd_params cpd;  // Cpd; zero otherwise
    gingr_icp_params icp;  // IcpCloud, IcpSurface; zero otherwise
};

enum class CorrespondenceError : int32_t {
    None = 0,
    BadFlavour,  // not one of the four
    CpdParams,   // Cpd: need 0 <= w < 1 and lambda > 0 (a null pointer included)
    IcpParams,   // IcpCloud, IcpSurface: need max_iterations >= 1 (a null pointer included)
};

// the rules, on a descriptor as built below (NaN fails every comparison: refused)
inline CorrespondenceError correspondence_error(const Correspondence &c) {
    switch (c.kind) {
        case Flavour::Cpd:
            return c.cpd.w >= 0.0 && c.cpd.w < 1.0 && c.cpd.lambda > 0.0 ? CorrespondenceError::None : CorrespondenceError::CpdParams;
        case Flavour::IcpCloud:
        case Flavour::IcpSurface:
            return c.icp.max_iterations >= 1 ? CorrespondenceError::None : CorrespondenceError::IcpParams;
        case Flavour::Pairs:
            return CorrespondenceError::None;
    }
    return CorrespondenceError::BadFlavour;
}

// The descriptor of the ABI's triple and what is wrong with it.  Only the parameters of the flavour are looked at (the other pointer
// may be anything); a null pointer where the flavour needs parameters leaves them zero, which the rules refuse -- the same answer the
// entry points have always given to a null and to a bad struct.
inline CorrespondenceError make_correspondence(int32_t flavour, const gingr_cpd_params *cp, const gingr_icp_params *ip, Correspondence *out) {
    *out = Correspondence{static_cast<Flavour>(flavour), gingr_cpd_params{0.0, 0.0}, gingr_icp_params{0.0, 0.0, 0}};
    if (out->kind == Flavour::Cpd && cp) out->cpd = *cp;
    if ((out->kind == Flavour::IcpCloud || out->kind == Flavour::IcpSurface) && ip) out->icp = *ip;
    return correspondence_error(*out);
}
inline Correspondence abi_correspondence(int32_t flavour, const gingr_cpd_params *cp, const gingr_icp_params *ip) {
    Correspondence c;
    (void)make_correspondence(flavour, cp, ip, &c);  // (check_correspondence reports what is wrong, behind the checks that come first)
    return c;
}

// ---- what follows from the flavour; `reversed`: gingr_fitter_set_correspondence_direction, which the pairs flavour and CPD ignore
// sigma2 of the next state follows ICP's schedule (ICP.scala:65, :96-99)
inline bool is_icp_schedule(const Correspondence &c) { return c.kind == Flavour::IcpCloud || c.kind == Flavour::IcpSurface; }
// what post_solve_kernel does about sigma2: 0 CPD's sums, 1 ICP's schedule, 2 kept (the pairs flavour: the caller's updateSigma2)
inline int32_t post_solve_sigma2_rule(const Correspondence &c) { return c.kind == Flavour::Cpd ? 0 : c.kind == Flavour::Pairs ? 2 : 1; }
inline bool needs_meshes(const Correspondence &c) { return c.kind == Flavour::IcpSurface; }
inline bool reversed_icp(const Correspondence &c, bool reversed) { return is_icp_schedule(c) && reversed; }
// row shards: the tests against the template need all of it (the surface flavour; the reversed direction of either ICP flavour)
inline bool needs_gathered_fit(const Correspondence &c, bool reversed) { return c.kind == Flavour::IcpSurface || reversed_icp(c, reversed); }
// row shards: phase 0 leaves something in exchange segment 0 (CPD's column sums; the others' correspondences are local to the rows)
inline bool exchanges_segment0(const Correspondence &c) { return c.kind == Flavour::Cpd; }
// row shards: the per-template-vertex sums of the reversed direction are totalled behind phase 0
inline bool exchanges_reversal_sums(const Correspondence &c, bool reversed) { return reversed_icp(c, reversed); }
// every row has the weight 1 / sigma2 (ICP.scala:90-92): the Gram matrix is the model's moment scaled, the observation is formed
// inside the right-hand-side sweep, the posterior mean can come from the model's eigen-decomposition
inline bool uniform_weights(const Correspondence &c, bool reversed, int32_t n_landmarks) {
    return c.kind == Flavour::IcpCloud && !reversed && n_landmarks == 0;
}
// the weights are 1 / sigma2 or 0 (forward surface ICP, ICP.scala:50): the Gram matrix may be the moment minus the zero-weight rows
inline bool zero_one_weights(const Correspondence &c, bool reversed) { return c.kind == Flavour::IcpSurface && !reversed; }
// gingr_fitter::Key::flavour: equal for two calls exactly when phases 0 and 1 of one state compute the same for both (the parameters
// of CPD are compared next to it; the pairs as they stand -- setting them forgets the memo, so the key need not describe them)
inline int memo_flavour_key(const Correspondence &c, int32_t surface_method, bool reversed) {
    if (c.kind == Flavour::Cpd) return 0;
    if (c.kind == Flavour::Pairs) return 3;
    return static_cast<int>(c.kind) + 4 * surface_method + 16 * (reversed ? 1 : 0);
}
