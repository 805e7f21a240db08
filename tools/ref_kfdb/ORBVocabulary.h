/*
 * A stand-in for the reference's include/ORBVocabulary.h, for tools/ref_kfdb: the two members KeyFrameDatabase calls.  score() hands the vectors to
 * the reference's own L1Scoring (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp, compiled unmodified), which is what TemplatedVocabulary::score does for
 * the ORB vocabulary (TF-IDF, L1 norm, L1 scoring).  AUTHORING TOOLING ONLY.
 */
#ifndef ORBVOCABULARY_H
#define ORBVOCABULARY_H

#include "Thirdparty/DBoW2/DBoW2/BowVector.h"
#include "Thirdparty/DBoW2/DBoW2/ScoringObject.h"

using namespace std;                             /* as TemplatedVocabulary.h:36 does behind the reference's header: KeyFrameDatabase.h writes `list` */

namespace Jetson_SLAM {

class ORBVocabulary {
public:
    explicit ORBVocabulary(unsigned int n_words) : n_words(n_words) {}
    unsigned int size() const { return n_words; }
    double score(const DBoW2::BowVector &a, const DBoW2::BowVector &b) const { return scoring.score(a, b); }

    unsigned int n_words;
    DBoW2::L1Scoring scoring;
};

}  // namespace Jetson_SLAM

#endif
