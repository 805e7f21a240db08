/* <opencv2/features2d/features2d.hpp> for tools/ref_culling: nothing of it is used. */
