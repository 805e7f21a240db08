/* A stand-in for the reference's include/ORBmatcher.h, for tools/ref_covis: src/KeyFrame.cpp includes it and uses nothing of it. */
#ifndef ORBMATCHER_H
#define ORBMATCHER_H
#endif
