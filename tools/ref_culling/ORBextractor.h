/* A stand-in for the reference's include/ORBextractor.h, for tools/ref_culling: include/KeyFrame.h includes it and uses nothing of it. */
#ifndef ORBEXTRACTOR_H
#define ORBEXTRACTOR_H
#endif
