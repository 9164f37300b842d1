// Probe build only (probe.hpp: NICE_PROBE_INC), inside the per-base
// launcher of fd2_part.hip: NICE_FD2_VD / NICE_FD2_LG / NICE_FD2_PERS /
// NICE_FD2_SIB ... select sweep instantiations of the FD kernel.
// FD2_BIG(flags): the base's big-field workgroups with the VD flags given.
#define FD2_BIG(...) launch_cfg<Cfg<B_, ND_, NE_, NE2_, 0, big_wg(B_), (__VA_ARGS__)>>(p, num_cus, s)
// FD2_VD_CASE(k, flags): knob value k + flags runs the flags (so the knob's
// number and the configuration cannot disagree).
#define FD2_VD_CASE(k, ...) case (k) + (__VA_ARGS__): return FD2_BIG(__VA_ARGS__)
// FD2_SIB40(flags, lg, m): b40, m sibling lanes at 512 threads.
#define FD2_SIB40(vdf, lg, m) launch_cfg<Cfg<B_, ND_, NE_, NE2_, 0, 512, (vdf), lg, 0, m>>(p, num_cus, s)
        // Small fields (< 1e7, 512-thread workgroups), b40 / b80: NICE_FD2_SMALLV
        // 1 = no low-digit table (limb 0 looked up in the pair table), 2 = the
        // same with limb 0 by VALU, 3 = no table at all (every limb by VALU)
        if constexpr (B_ == 40 || B_ == 80) {
            if (wg512) {
                switch ((int)probe_knob("NICE_FD2_SMALLV", 0)) {
                case 1: return launch_cfg<Cfg<B_, ND_, NE_, NE2_, 0, 512, valu_limbs(B_) | vd::NOLOW>>(p, num_cus, s);
                case 2: return launch_cfg<Cfg<B_, ND_, NE_, NE2_, 0, 512, valu_limbs(B_) | vd::NOLOW | vd::LIMB0>>(p, num_cus, s);
                case 3: return launch_cfg<Cfg<B_, ND_, NE_, NE2_, 0, 512, vd::NOTAB>>(p, num_cus, s);
                default: break;
                }
            }
        }
        // VALU-decoded limb sweep (scripts/vd_sweep.py): NICE_FD2_VD = 100 + VD
        switch ((int)probe_knob("NICE_FD2_VD", 0)) {
        FD2_VD_CASE(100, 0);
        FD2_VD_CASE(100, vd::c(1));
        FD2_VD_CASE(100, vd::c(2));
        FD2_VD_CASE(100, vd::c(3));
        FD2_VD_CASE(100, vd::s(1) | vd::c(1));
        FD2_VD_CASE(100, vd::s(1) | vd::c(2));
        FD2_VD_CASE(100, vd::LIMB0);
        FD2_VD_CASE(100, vd::LIMB0 | vd::c(1));
        FD2_VD_CASE(100, vd::LIMB0 | vd::c(2));
        default: break;
        }
        // b65..80: VALU-decoded limbs just below the top stepped limb
        // (vd::BELOW): NICE_FD2_VD = 100 + VD as above
        if constexpr (mask_words(B_) == 3) {
            constexpr int LB = vd::LIMB0 | vd::BELOW;
            switch ((int)probe_knob("NICE_FD2_VD", 0)) {
            FD2_VD_CASE(100, LB | vd::c(1));
            FD2_VD_CASE(100, LB | vd::c(2));
            FD2_VD_CASE(100, LB | vd::s(1));
            FD2_VD_CASE(100, LB | vd::c(3));
            FD2_VD_CASE(100, LB | vd::s(1) | vd::c(1));
            FD2_VD_CASE(100, LB | vd::s(1) | vd::c(2));
            FD2_VD_CASE(100, LB | vd::c(4));
            FD2_VD_CASE(100, LB | vd::s(1) | vd::c(3));
            default: break;
            }
        }
        // Two-word bases: k limbs below the top stepped ones by VALU (vd::BELOW,
        // keeping the base's low-digit-table mode): NICE_FD2_VD = 6000 + k
        if constexpr (mask_words(B_) == 2) {
            constexpr int KEEP = valu_limbs(B_) & vd::SIDE;
            switch ((int)probe_knob("NICE_FD2_VD", 0)) {
            case 6000 + vd::c(1): return FD2_BIG(KEEP | vd::BELOW | vd::c(1));
            case 6000 + vd::c(2): return FD2_BIG(KEEP | vd::BELOW | vd::c(2));
            case 6000 + vd::c(3): return FD2_BIG(KEEP | vd::BELOW | vd::c(3));
            case 6000 + (vd::s(1) | vd::c(1)): return FD2_BIG(KEEP | vd::BELOW | vd::s(1) | vd::c(1));
            default: break;
            }
        }
        // Any base with VALU-decoded top limbs: the same count just below the
        // top stepped limbs instead (vd::BELOW): NICE_FD2_VD = 5000
        if constexpr ((valu_limbs(B_) & vd::LIMBS) != 0 && (valu_limbs(B_) & vd::BELOW) == 0) {
            if ((int)probe_knob("NICE_FD2_VD", 0) == 5000) return FD2_BIG(valu_limbs(B_) | vd::BELOW);
        }
        // Low-digit table with a side table of carries (Cfg::LSDX, b59..64):
        // NICE_FD2_VD = 1100 + VD, VD = the VALU-decoded top limbs
        if constexpr (mask_words(B_) == 2 && !lsd_w1_fits(B_)) {
            switch ((int)probe_knob("NICE_FD2_VD", 0)) {
            case 1100: return FD2_BIG(vd::SIDE);
            case 1100 + vd::c(1): return FD2_BIG(vd::SIDE | vd::c(1));
            case 1100 + vd::c(2): return FD2_BIG(vd::SIDE | vd::c(2));
            case 1100 + vd::c(3): return FD2_BIG(vd::SIDE | vd::c(3));
            case 1100 + (vd::s(1) | vd::c(1)): return FD2_BIG(vd::SIDE | vd::s(1) | vd::c(1));
            case 1100 + (vd::s(1) | vd::c(2)): return FD2_BIG(vd::SIDE | vd::s(1) | vd::c(2));
            default: break;
            }
        }
        // Sibling lanes (Cfg::SIB) A/B: NICE_FD2_SIB = 1: the round-4 kernel
        // (no siblings) on every sibling base; on b40 31 / 131 / 132 / 141 /
        // 142 / 143 / 144 / 121: M = 3 or 2 siblings at the VALU decode /
        // lookup grouping in the cases
        if constexpr (B_ >= 40 && B_ <= 55) {
            if (!wg512 && probe_knob("NICE_FD2_SIB", 0) == 1)
                return launch_cfg<RegularBig<B_, ND_, NE_, NE2_>>(p, num_cus, s);
        }
        if constexpr (B_ == 40) {
            constexpr int VL = valu_limbs_big(B_, ND_, NE_);
            switch ((int)probe_knob("NICE_FD2_SIB", 0)) {
            case 31: return FD2_SIB40(VL, 1, 3);
            case 131: return FD2_SIB40(0, 1, 3);
            case 132: return FD2_SIB40(0, 100, 3);
            case 141: return FD2_SIB40(vd::LOWEST | vd::c(1), 1, 3);
            case 142: return FD2_SIB40(vd::LOWEST | vd::c(1), 100, 3);
            case 143: return FD2_SIB40(vd::LOWEST | vd::c(2), 1, 3);
            case 144: return FD2_SIB40(vd::LOWEST | vd::s(1) | vd::c(1), 1, 3);
            case 121: return FD2_SIB40(vd::LOWEST | vd::c(1), 1, 2);
            // 142 / 131 with the limb arithmetic on the f32 FMA pipe (vd::FMA):
            // the production kernels, 142 / 131 being their integer forms
            case 242: return FD2_SIB40(vd::LOWEST | vd::c(1) | vd::FMA, 100, 3);
            case 231: return FD2_SIB40(vd::FMA, 1, 3);
            default: break;
            }
        }
        // Persistent grid A/B (NICE_FD2_PERS = 1: on, 2: off; 3 / 4: 1024-thread
        // workgroups with / without it, where the LDS and VGPRs allow one)
        if constexpr (waves_at(B_, 1024) >= 4) {
            switch ((int)probe_knob("NICE_FD2_PERS", 0)) {
            case 3: return launch_cfg<Cfg<B_, ND_, NE_, NE2_, 0, 1024, valu_limbs(B_), -1, 1>>(p, num_cus, s);
            case 4: return launch_cfg<Cfg<B_, ND_, NE_, NE2_, 0, 1024, valu_limbs(B_), -1, 0>>(p, num_cus, s);
            default: break;
            }
        }
        switch ((int)probe_knob("NICE_FD2_PERS", 0)) {
        case 1:
            return wg512 ? launch_cfg<Cfg<B_, ND_, NE_, NE2_, 0, 512, valu_limbs(B_), -1, 1>>(p, num_cus, s)
                         : launch_cfg<Cfg<B_, ND_, NE_, NE2_, 0, big_wg(B_), valu_limbs(B_), -1, 1>>(p, num_cus, s);
        case 2:
            return wg512 ? launch_cfg<Cfg<B_, ND_, NE_, NE2_, 0, 512, valu_limbs(B_), -1, 0>>(p, num_cus, s)
                         : launch_cfg<Cfg<B_, ND_, NE_, NE2_, 0, big_wg(B_), valu_limbs(B_), -1, 0>>(p, num_cus, s);
        default: break;
        }
        // Lookup-group sweep of the three-mask-word bases (NICE_FD2_LG = LG,
        // at the production VALU-decoded limbs of fields >= 1e7)
        if constexpr (mask_words(B_) == 3) {
            constexpr int VL = valu_limbs_big(B_, ND_, NE_), WGB = big_wg(B_);
            switch ((int)probe_knob("NICE_FD2_LG", 100000)) {
            case 0: return launch_cfg<Cfg<B_, ND_, NE_, NE2_, 0, WGB, VL, 0>>(p, num_cus, s);
            case 5: return launch_cfg<Cfg<B_, ND_, NE_, NE2_, 0, WGB, VL, 5>>(p, num_cus, s);
            case 6: return launch_cfg<Cfg<B_, ND_, NE_, NE2_, 0, WGB, VL, 6>>(p, num_cus, s);
            case 7: return launch_cfg<Cfg<B_, ND_, NE_, NE2_, 0, WGB, VL, 7>>(p, num_cus, s);
            case 8: return launch_cfg<Cfg<B_, ND_, NE_, NE2_, 0, WGB, VL, 8>>(p, num_cus, s);
            case 10: return launch_cfg<Cfg<B_, ND_, NE_, NE2_, 0, WGB, VL, 10>>(p, num_cus, s);
            case 12: return launch_cfg<Cfg<B_, ND_, NE_, NE2_, 0, WGB, VL, 12>>(p, num_cus, s);
            default: break;
            }
        }
#undef FD2_BIG
#undef FD2_VD_CASE
#undef FD2_SIB40
