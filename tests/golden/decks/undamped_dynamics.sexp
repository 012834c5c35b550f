;; -*- Mode: lisp; -*-
(task
 (model :name COMPRESSIBLE_NEOHOOKEAN
        (model-parameters :mu 100 :lambda 100))
 (solution :desired-tolerance 1e-08 :task-type CARTESIAN3D :load-increments-count 1 :modified-newton yes :max-newton-count 20
   (element-type :gauss-nodes-count 1 :name TETRAHEDRA4 :nodes-count 4)
   (slae-solver :type CG :tolerance 1e-14 :max-iterations 20000)
   (line-search :max 0)
   (arc-length :max 0)
   (dynamics :steps 3 :dt 0.0625 :beta 0.25 :gamma 0.5 :dlambda 1 :density 1.5))
 (input-data
  (geometry
   (nodes
    (0 1 0)
    (1 1 0)
    (0 1 1)
    (1 1 1)
    (0 4 0)
    (1 4 0)
    (0 4 1)
    (1 4 1)
    (0 7 0)
    (1 7 0)
    (0 7 1)
    (1 7 1))
   (elements
    (0 1 5 7)
    (0 3 1 7)
    (0 5 4 7)
    (0 4 6 7)
    (0 2 3 7)
    (0 6 2 7)
    (4 5 9 11)
    (4 7 5 11)
    (4 9 8 11)
    (4 8 10 11)
    (4 6 7 11)
    (4 10 6 11)))
  (boundary-conditions
   (prescribed-displacements
    (presc-node :y 0 :x 0 :z 0 :type 7 :node-id 0)
    (presc-node :y 0 :x 0 :z 0 :type 7 :node-id 1)
    (presc-node :y 0 :x 0 :z 0 :type 7 :node-id 2)
    (presc-node :y 0 :x 0 :z 0 :type 7 :node-id 3)
    (presc-node :y 0.050000000000000003 :x 0 :z 0 :type 7 :node-id 8)
    (presc-node :y 0.050000000000000003 :x 0 :z 0 :type 7 :node-id 9)
    (presc-node :y 0.050000000000000003 :x 0 :z 0 :type 7 :node-id 10)
    (presc-node :y 0.050000000000000003 :x 0 :z 0 :type 7 :node-id 11))
   (body-force :x 0 :y 0 :z -2))))
