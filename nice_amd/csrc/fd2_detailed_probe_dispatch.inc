// Probe build only (probe.hpp: NICE_PROBE_INC), inside launch_segment
// (fd2_detailed.hip): NICE_FD2_PROBE selects a bottleneck-probe or sweep
// instantiation of the FD kernel for the segment's limb combo.
    if (probe && p.base == 40 && c.nd == 4 && c.ne == 8 && c.ne2 == 5) {
        if (probe == 1) return launch_cfg<Cfg<40, 4, 8, 5, 1>>(p, num_cus, s);
        if (probe == 2) return launch_cfg<Cfg<40, 4, 8, 5, 2>>(p, num_cus, s);
        if (probe == 3) return launch_cfg<Cfg<40, 4, 8, 5, 3>>(p, num_cus, s);
        if (probe == 4) return launch_cfg<Cfg<40, 4, 8, 5, 4>>(p, num_cus, s);
        // Workgroup-size sweep (profiles/r01/fd2_wg_sweep.log): 512 and 768
        // (6 waves/SIMD) tie at 2.56-2.58 ms, 1024 (8 waves, spills) 2.59,
        // 896 (7 waves) 2.85-2.92, 640 (5 waves) 3.18.
        if (probe == 6) return launch_cfg<Cfg<40, 4, 8, 5, 0, 768>>(p, num_cus, s);
        if (probe == 7) return launch_cfg<Cfg<40, 4, 8, 5, 0, 1024>>(p, num_cus, s);
        if (probe == 5) return launch_cfg<Cfg<40, 4, 8, 5, 0, 896>>(p, num_cus, s);
        if (probe == 8) return launch_cfg<Cfg<40, 4, 8, 5, 0, 512, vd::c(1)>>(p, num_cus, s);
        if (probe == 9) return launch_cfg<Cfg<40, 4, 8, 5, 0, 512, vd::s(1) | vd::c(1)>>(p, num_cus, s);
    }
    // b80 VALU-decoded limbs (probe 30 + VD: 31..34 = 1..4 top C limbs, 47 =
    // 1 C + 1 S, 48 = 2 C + 1 S), 1024-thread workgroups, main combo
    if (probe >= 30 && p.base == 80 && c.nd == 8 && c.ne == 16 && c.ne2 == 9) {
        if (probe == 31) return launch_cfg<Cfg<80, 8, 16, 9, 0, 1024, vd::c(1)>>(p, num_cus, s);
        if (probe == 32) return launch_cfg<Cfg<80, 8, 16, 9, 0, 1024, vd::c(2)>>(p, num_cus, s);
        if (probe == 33) return launch_cfg<Cfg<80, 8, 16, 9, 0, 1024, vd::c(3)>>(p, num_cus, s);
        if (probe == 34) return launch_cfg<Cfg<80, 8, 16, 9, 0, 1024, vd::c(4)>>(p, num_cus, s);
        if (probe == 36) return launch_cfg<Cfg<80, 8, 16, 9, 0, 1024, vd::c(6)>>(p, num_cus, s);
        if (probe == 47) return launch_cfg<Cfg<80, 8, 16, 9, 0, 1024, vd::s(1) | vd::c(1)>>(p, num_cus, s);
        if (probe == 48) return launch_cfg<Cfg<80, 8, 16, 9, 0, 1024, vd::s(1) | vd::c(2)>>(p, num_cus, s);
    }
    if (probe >= 30 && p.base == 64 && c.nd == 7 && c.ne == 13 && c.ne2 == 7) {
        if (probe == 31) return launch_cfg<Cfg<64, 7, 13, 7, 0, 512, vd::c(1)>>(p, num_cus, s);
        if (probe == 32) return launch_cfg<Cfg<64, 7, 13, 7, 0, 512, vd::c(2)>>(p, num_cus, s);
        if (probe == 33) return launch_cfg<Cfg<64, 7, 13, 7, 0, 512, vd::c(3)>>(p, num_cus, s);
        if (probe == 47) return launch_cfg<Cfg<64, 7, 13, 7, 0, 512, vd::s(1) | vd::c(1)>>(p, num_cus, s);
        if (probe == 48) return launch_cfg<Cfg<64, 7, 13, 7, 0, 512, vd::s(1) | vd::c(2)>>(p, num_cus, s);
    }
    if (probe >= 30 && p.base == 68 && c.nd == 7 && c.ne == 14 && c.ne2 == 7) {
        if (probe == 31) return launch_cfg<Cfg<68, 7, 14, 7, 0, 1024, vd::c(1)>>(p, num_cus, s);
        if (probe == 32) return launch_cfg<Cfg<68, 7, 14, 7, 0, 1024, vd::c(2)>>(p, num_cus, s);
        if (probe == 47) return launch_cfg<Cfg<68, 7, 14, 7, 0, 1024, vd::s(1) | vd::c(1)>>(p, num_cus, s);
    }
