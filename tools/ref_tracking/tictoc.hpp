/* A stand-in for the reference's include/tictoc.hpp, for tools/ref_tracking: a stopwatch that src/Tracking.cpp starts and never reads. */
#ifndef JSORB_REF_TRACKING_TICTOC_HPP
#define JSORB_REF_TRACKING_TICTOC_HPP

class tictoc {
public:
    void tic() {}
    float toc() { return 0.0f; }
    void toc_print() {}
};

#endif
