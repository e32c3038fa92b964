/* Empty on purpose: the reference's src/kernels.cu includes <glm/glm.hpp> and uses nothing from it. */
