// The step loop of a persistent scan kernel: the kernel's step body M3T_STEP_FILE (a string literal) written out twice, because the
// inline-asm prefetch needs two register sets whose names are fixed at compile time -- even steps use set A and fill B, odd steps the
// reverse.  STEPV = the step index, PARV = its parity as a constant, CUR(x) / NXT(x) = the set in use / being filled.  An odd T leaves
// between the two bodies.
    for (int step2 = 0; step2 < T; step2 += 2) {
#define STEPV step2
#define PARV 0
#define CUR(x) x##A
#define NXT(x) x##B
#include M3T_STEP_FILE
#undef STEPV
#undef PARV
#undef CUR
#undef NXT
        if (step2 + 1 >= T) break;
#define STEPV (step2 + 1)
#define PARV 1
#define CUR(x) x##B
#define NXT(x) x##A
#include M3T_STEP_FILE
#undef STEPV
#undef PARV
#undef CUR
#undef NXT
    }
#undef M3T_STEP_FILE
