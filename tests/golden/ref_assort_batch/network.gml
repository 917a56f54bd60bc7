graph
[
	directed 0
	node
	[
		id 0
		extid 2
		group 2
		bridgeness 1.00556
		influence 19
		degree 19
	]
	node
	[
		id 1
		extid 1
		group 3
		bridgeness 12.96607
		influence 16
		degree 29
	]
	node
	[
		id 2
		extid 6
		group 2
		bridgeness 1.87392
		influence 20
		degree 22
	]
	node
	[
		id 3
		extid 10
		group 2
		bridgeness 1.79944
		influence 22
		degree 22
	]
	node
	[
		id 4
		extid 11
		group 2
		bridgeness 10.78963
		influence 13
		degree 23
	]
	node
	[
		id 5
		extid 12
		group 2
		bridgeness 0.52742
		influence 19
		degree 19
	]
	node
	[
		id 6
		extid 13
		group 2
		bridgeness 0.50722
		influence 18
		degree 18
	]
	node
	[
		id 7
		extid 15
		group 2
		bridgeness 0.02710
		influence 19
		degree 19
	]
	node
	[
		id 8
		extid 16
		group 2
		bridgeness 2.60587
		influence 20
		degree 23
	]
	node
	[
		id 9
		extid 18
		group 2
		bridgeness 0.02832
		influence 19
		degree 19
	]
	node
	[
		id 10
		extid 22
		group 3
		bridgeness 3.04289
		influence 26
		degree 26
	]
	node
	[
		id 11
		extid 24
		group 3
		bridgeness 12.57217
		influence 16
		degree 25
	]
	node
	[
		id 12
		extid 26
		group 3
		bridgeness 0.03588
		influence 23
		degree 23
	]
	node
	[
		id 13
		extid 27
		group 3
		bridgeness 2.09898
		influence 23
		degree 25
	]
	node
	[
		id 14
		extid 28
		group 3
		bridgeness 0.59467
		influence 23
		degree 23
	]
	node
	[
		id 15
		extid 30
		group 3
		bridgeness 2.03937
		influence 25
		degree 25
	]
	node
	[
		id 16
		extid 32
		group 3
		bridgeness 0.02913
		influence 21
		degree 21
	]
	node
	[
		id 17
		extid 33
		group 3
		bridgeness 0.66916
		influence 24
		degree 24
	]
	node
	[
		id 18
		extid 36
		group 3
		bridgeness 3.67964
		influence 22
		degree 26
	]
	node
	[
		id 19
		extid 37
		group 3
		bridgeness 1.96145
		influence 23
		degree 25
	]
	node
	[
		id 20
		extid 40
		group 3
		bridgeness 2.75032
		influence 23
		degree 25
	]
	node
	[
		id 21
		extid 41
		group 3
		bridgeness 2.14234
		influence 23
		degree 24
	]
	node
	[
		id 22
		extid 43
		group 3
		bridgeness 0.65243
		influence 23
		degree 23
	]
	node
	[
		id 23
		extid 44
		group 3
		bridgeness 0.63456
		influence 23
		degree 23
	]
	node
	[
		id 24
		extid 74
		group 0
		bridgeness 3.12797
		influence 12
		degree 17
	]
	node
	[
		id 25
		extid 3
		group 2
		bridgeness 1.13787
		influence 21
		degree 21
	]
	node
	[
		id 26
		extid 5
		group 2
		bridgeness 1.78156
		influence 22
		degree 22
	]
	node
	[
		id 27
		extid 7
		group 2
		bridgeness 0.02496
		influence 17
		degree 17
	]
	node
	[
		id 28
		extid 8
		group 2
		bridgeness 15.76785
		influence 15
		degree 33
	]
	node
	[
		id 29
		extid 14
		group 2
		bridgeness 0.49948
		influence 18
		degree 18
	]
	node
	[
		id 30
		extid 17
		group 2
		bridgeness 1.03729
		influence 20
		degree 20
	]
	node
	[
		id 31
		extid 19
		group 2
		bridgeness 3.15785
		influence 19
		degree 22
	]
	node
	[
		id 32
		extid 20
		group 2
		bridgeness 15.49814
		influence 16
		degree 34
	]
	node
	[
		id 33
		extid 21
		group 2
		bridgeness 7.98263
		influence 11
		degree 18
	]
	node
	[
		id 34
		extid 64
		group 1
		bridgeness 5.81182
		influence 25
		degree 28
	]
	node
	[
		id 35
		extid 4
		group 2
		bridgeness 0.02460
		influence 17
		degree 17
	]
	node
	[
		id 36
		extid 9
		group 2
		bridgeness 10.66762
		influence 14
		degree 26
	]
	node
	[
		id 37
		extid 56
		group 1
		bridgeness 4.10611
		influence 24
		degree 26
	]
	node
	[
		id 38
		extid 47
		group 0
		bridgeness 8.88106
		influence 9
		degree 20
	]
	node
	[
		id 39
		extid 49
		group 1
		bridgeness 5.50757
		influence 24
		degree 26
	]
	node
	[
		id 40
		extid 50
		group 1
		bridgeness 0.55744
		influence 22
		degree 22
	]
	node
	[
		id 41
		extid 52
		group 1
		bridgeness 1.66516
		influence 25
		degree 25
	]
	node
	[
		id 42
		extid 53
		group 0
		bridgeness 16.29839
		influence 12
		degree 28
	]
	node
	[
		id 43
		extid 54
		group 1
		bridgeness 3.02475
		influence 22
		degree 24
	]
	node
	[
		id 44
		extid 55
		group 1
		bridgeness 13.35643
		influence 22
		degree 32
	]
	node
	[
		id 45
		extid 59
		group 1
		bridgeness 0.03084
		influence 21
		degree 21
	]
	node
	[
		id 46
		extid 63
		group 1
		bridgeness 7.20065
		influence 24
		degree 28
	]
	node
	[
		id 47
		extid 45
		group 1
		bridgeness 2.37327
		influence 26
		degree 27
	]
	node
	[
		id 48
		extid 51
		group 1
		bridgeness 2.31777
		influence 25
		degree 25
	]
	node
	[
		id 49
		extid 58
		group 1
		bridgeness 1.62054
		influence 23
		degree 23
	]
	node
	[
		id 50
		extid 65
		group 1
		bridgeness 3.07958
		influence 23
		degree 25
	]
	node
	[
		id 51
		extid 29
		group 3
		bridgeness 2.17576
		influence 24
		degree 24
	]
	node
	[
		id 52
		extid 35
		group 3
		bridgeness 12.96765
		influence 18
		degree 30
	]
	node
	[
		id 53
		extid 67
		group 0
		bridgeness 3.25509
		influence 16
		degree 16
	]
	node
	[
		id 54
		extid 73
		group 0
		bridgeness 1.82791
		influence 13
		degree 14
	]
	node
	[
		id 55
		extid 75
		group 0
		bridgeness 2.16274
		influence 13
		degree 14
	]
	node
	[
		id 56
		extid 57
		group 1
		bridgeness 0.03094
		influence 22
		degree 22
	]
	node
	[
		id 57
		extid 60
		group 1
		bridgeness 1.62092
		influence 23
		degree 23
	]
	node
	[
		id 58
		extid 61
		group 1
		bridgeness 3.04261
		influence 26
		degree 26
	]
	node
	[
		id 59
		extid 66
		group 1
		bridgeness 2.07770
		influence 23
		degree 23
	]
	node
	[
		id 60
		extid 70
		group 0
		bridgeness 3.93917
		influence 15
		degree 17
	]
	node
	[
		id 61
		extid 23
		group 1
		bridgeness 17.11174
		influence 21
		degree 39
	]
	node
	[
		id 62
		extid 25
		group 3
		bridgeness 1.75389
		influence 21
		degree 22
	]
	node
	[
		id 63
		extid 31
		group 3
		bridgeness 3.30101
		influence 22
		degree 25
	]
	node
	[
		id 64
		extid 34
		group 3
		bridgeness 1.36204
		influence 23
		degree 24
	]
	node
	[
		id 65
		extid 38
		group 3
		bridgeness 2.16492
		influence 23
		degree 24
	]
	node
	[
		id 66
		extid 39
		group 3
		bridgeness 0.03138
		influence 22
		degree 22
	]
	node
	[
		id 67
		extid 42
		group 3
		bridgeness 0.02996
		influence 21
		degree 21
	]
	node
	[
		id 68
		extid 46
		group 1
		bridgeness 1.37501
		influence 24
		degree 24
	]
	node
	[
		id 69
		extid 48
		group 1
		bridgeness 8.34213
		influence 17
		degree 22
	]
	node
	[
		id 70
		extid 62
		group 1
		bridgeness 10.69172
		influence 13
		degree 22
	]
	node
	[
		id 71
		extid 68
		group 0
		bridgeness 6.11676
		influence 16
		degree 19
	]
	node
	[
		id 72
		extid 72
		group 0
		bridgeness 4.35682
		influence 17
		degree 18
	]
	node
	[
		id 73
		extid 69
		group 0
		bridgeness 5.08301
		influence 15
		degree 18
	]
	node
	[
		id 74
		extid 71
		group 0
		bridgeness 1.71069
		influence 13
		degree 13
	]
	edge
	[
		source 0
		target 1
		color 2
	]
	edge
	[
		source 0
		target 2
		color 2
	]
	edge
	[
		source 0
		target 3
		color 2
	]
	edge
	[
		source 0
		target 4
		color 2
	]
	edge
	[
		source 0
		target 5
		color 2
	]
	edge
	[
		source 0
		target 6
		color 2
	]
	edge
	[
		source 0
		target 7
		color 2
	]
	edge
	[
		source 0
		target 8
		color 2
	]
	edge
	[
		source 0
		target 9
		color 2
	]
	edge
	[
		source 0
		target 25
		color 2
	]
	edge
	[
		source 0
		target 26
		color 2
	]
	edge
	[
		source 0
		target 27
		color 2
	]
	edge
	[
		source 0
		target 28
		color 2
	]
	edge
	[
		source 0
		target 29
		color 2
	]
	edge
	[
		source 0
		target 30
		color 2
	]
	edge
	[
		source 0
		target 31
		color 2
	]
	edge
	[
		source 0
		target 32
		color 2
	]
	edge
	[
		source 0
		target 33
		color 2
	]
	edge
	[
		source 1
		target 2
		color 2
	]
	edge
	[
		source 1
		target 3
		color 2
	]
	edge
	[
		source 1
		target 4
		color 2
	]
	edge
	[
		source 1
		target 5
		color 2
	]
	edge
	[
		source 1
		target 6
		color 2
	]
	edge
	[
		source 1
		target 7
		color 2
	]
	edge
	[
		source 1
		target 8
		color 2
	]
	edge
	[
		source 1
		target 9
		color 2
	]
	edge
	[
		source 1
		target 10
		color 3
	]
	edge
	[
		source 1
		target 11
		color 3
	]
	edge
	[
		source 1
		target 12
		color 3
	]
	edge
	[
		source 1
		target 13
		color 3
	]
	edge
	[
		source 1
		target 14
		color 3
	]
	edge
	[
		source 1
		target 15
		color 3
	]
	edge
	[
		source 1
		target 16
		color 3
	]
	edge
	[
		source 1
		target 17
		color 3
	]
	edge
	[
		source 1
		target 18
		color 3
	]
	edge
	[
		source 1
		target 19
		color 3
	]
	edge
	[
		source 1
		target 20
		color 3
	]
	edge
	[
		source 1
		target 21
		color 3
	]
	edge
	[
		source 1
		target 22
		color 3
	]
	edge
	[
		source 1
		target 23
		color 3
	]
	edge
	[
		source 1
		target 24
		color 2
	]
	edge
	[
		source 1
		target 26
		color 2
	]
	edge
	[
		source 1
		target 27
		color 2
	]
	edge
	[
		source 1
		target 64
		color 3
	]
	edge
	[
		source 1
		target 65
		color 3
	]
	edge
	[
		source 2
		target 3
		color 2
	]
	edge
	[
		source 2
		target 4
		color 2
	]
	edge
	[
		source 2
		target 5
		color 2
	]
	edge
	[
		source 2
		target 6
		color 2
	]
	edge
	[
		source 2
		target 7
		color 2
	]
	edge
	[
		source 2
		target 8
		color 2
	]
	edge
	[
		source 2
		target 9
		color 2
	]
	edge
	[
		source 2
		target 25
		color 2
	]
	edge
	[
		source 2
		target 26
		color 2
	]
	edge
	[
		source 2
		target 27
		color 2
	]
	edge
	[
		source 2
		target 28
		color 2
	]
	edge
	[
		source 2
		target 29
		color 2
	]
	edge
	[
		source 2
		target 30
		color 2
	]
	edge
	[
		source 2
		target 31
		color 2
	]
	edge
	[
		source 2
		target 32
		color 2
	]
	edge
	[
		source 2
		target 35
		color 2
	]
	edge
	[
		source 2
		target 36
		color 2
	]
	edge
	[
		source 3
		target 5
		color 2
	]
	edge
	[
		source 3
		target 6
		color 2
	]
	edge
	[
		source 3
		target 7
		color 2
	]
	edge
	[
		source 3
		target 8
		color 2
	]
	edge
	[
		source 3
		target 9
		color 2
	]
	edge
	[
		source 3
		target 25
		color 2
	]
	edge
	[
		source 3
		target 26
		color 2
	]
	edge
	[
		source 3
		target 27
		color 2
	]
	edge
	[
		source 3
		target 28
		color 2
	]
	edge
	[
		source 3
		target 29
		color 2
	]
	edge
	[
		source 3
		target 30
		color 2
	]
	edge
	[
		source 3
		target 31
		color 2
	]
	edge
	[
		source 3
		target 32
		color 2
	]
	edge
	[
		source 3
		target 33
		color 2
	]
	edge
	[
		source 3
		target 35
		color 2
	]
	edge
	[
		source 3
		target 36
		color 2
	]
	edge
	[
		source 4
		target 7
		color 2
	]
	edge
	[
		source 4
		target 8
		color 2
	]
	edge
	[
		source 4
		target 9
		color 2
	]
	edge
	[
		source 4
		target 24
		color 0
	]
	edge
	[
		source 4
		target 25
		color 2
	]
	edge
	[
		source 4
		target 28
		color 2
	]
	edge
	[
		source 4
		target 29
		color 2
	]
	edge
	[
		source 4
		target 30
		color 2
	]
	edge
	[
		source 4
		target 31
		color 2
	]
	edge
	[
		source 4
		target 32
		color 2
	]
	edge
	[
		source 4
		target 44
		color 0
	]
	edge
	[
		source 4
		target 53
		color 0
	]
	edge
	[
		source 4
		target 54
		color 0
	]
	edge
	[
		source 4
		target 55
		color 0
	]
	edge
	[
		source 4
		target 71
		color 0
	]
	edge
	[
		source 5
		target 6
		color 2
	]
	edge
	[
		source 5
		target 7
		color 2
	]
	edge
	[
		source 5
		target 8
		color 2
	]
	edge
	[
		source 5
		target 9
		color 2
	]
	edge
	[
		source 5
		target 25
		color 2
	]
	edge
	[
		source 5
		target 26
		color 2
	]
	edge
	[
		source 5
		target 27
		color 2
	]
	edge
	[
		source 5
		target 29
		color 2
	]
	edge
	[
		source 5
		target 30
		color 2
	]
	edge
	[
		source 5
		target 31
		color 2
	]
	edge
	[
		source 5
		target 32
		color 2
	]
	edge
	[
		source 5
		target 33
		color 2
	]
	edge
	[
		source 5
		target 35
		color 2
	]
	edge
	[
		source 5
		target 36
		color 2
	]
	edge
	[
		source 6
		target 7
		color 2
	]
	edge
	[
		source 6
		target 8
		color 2
	]
	edge
	[
		source 6
		target 9
		color 2
	]
	edge
	[
		source 6
		target 25
		color 2
	]
	edge
	[
		source 6
		target 26
		color 2
	]
	edge
	[
		source 6
		target 27
		color 2
	]
	edge
	[
		source 6
		target 29
		color 2
	]
	edge
	[
		source 6
		target 30
		color 2
	]
	edge
	[
		source 6
		target 31
		color 2
	]
	edge
	[
		source 6
		target 33
		color 2
	]
	edge
	[
		source 6
		target 35
		color 2
	]
	edge
	[
		source 6
		target 36
		color 2
	]
	edge
	[
		source 7
		target 8
		color 2
	]
	edge
	[
		source 7
		target 9
		color 2
	]
	edge
	[
		source 7
		target 25
		color 2
	]
	edge
	[
		source 7
		target 26
		color 2
	]
	edge
	[
		source 7
		target 27
		color 2
	]
	edge
	[
		source 7
		target 28
		color 2
	]
	edge
	[
		source 7
		target 29
		color 2
	]
	edge
	[
		source 7
		target 30
		color 2
	]
	edge
	[
		source 7
		target 31
		color 2
	]
	edge
	[
		source 7
		target 33
		color 2
	]
	edge
	[
		source 7
		target 35
		color 2
	]
	edge
	[
		source 7
		target 36
		color 2
	]
	edge
	[
		source 8
		target 9
		color 2
	]
	edge
	[
		source 8
		target 25
		color 2
	]
	edge
	[
		source 8
		target 26
		color 2
	]
	edge
	[
		source 8
		target 27
		color 2
	]
	edge
	[
		source 8
		target 28
		color 2
	]
	edge
	[
		source 8
		target 29
		color 2
	]
	edge
	[
		source 8
		target 30
		color 2
	]
	edge
	[
		source 8
		target 31
		color 2
	]
	edge
	[
		source 8
		target 32
		color 2
	]
	edge
	[
		source 8
		target 35
		color 2
	]
	edge
	[
		source 8
		target 36
		color 2
	]
	edge
	[
		source 9
		target 25
		color 2
	]
	edge
	[
		source 9
		target 26
		color 2
	]
	edge
	[
		source 9
		target 27
		color 2
	]
	edge
	[
		source 9
		target 29
		color 2
	]
	edge
	[
		source 9
		target 30
		color 2
	]
	edge
	[
		source 9
		target 31
		color 2
	]
	edge
	[
		source 9
		target 32
		color 2
	]
	edge
	[
		source 9
		target 33
		color 2
	]
	edge
	[
		source 9
		target 35
		color 2
	]
	edge
	[
		source 9
		target 36
		color 2
	]
	edge
	[
		source 10
		target 11
		color 3
	]
	edge
	[
		source 10
		target 12
		color 3
	]
	edge
	[
		source 10
		target 13
		color 3
	]
	edge
	[
		source 10
		target 14
		color 3
	]
	edge
	[
		source 10
		target 15
		color 3
	]
	edge
	[
		source 10
		target 16
		color 3
	]
	edge
	[
		source 10
		target 17
		color 3
	]
	edge
	[
		source 10
		target 18
		color 3
	]
	edge
	[
		source 10
		target 19
		color 3
	]
	edge
	[
		source 10
		target 20
		color 3
	]
	edge
	[
		source 10
		target 21
		color 3
	]
	edge
	[
		source 10
		target 22
		color 3
	]
	edge
	[
		source 10
		target 23
		color 3
	]
	edge
	[
		source 10
		target 51
		color 3
	]
	edge
	[
		source 10
		target 52
		color 3
	]
	edge
	[
		source 10
		target 61
		color 3
	]
	edge
	[
		source 10
		target 62
		color 3
	]
	edge
	[
		source 10
		target 63
		color 3
	]
	edge
	[
		source 10
		target 64
		color 3
	]
	edge
	[
		source 10
		target 65
		color 3
	]
	edge
	[
		source 10
		target 66
		color 3
	]
	edge
	[
		source 10
		target 67
		color 3
	]
	edge
	[
		source 11
		target 12
		color 3
	]
	edge
	[
		source 11
		target 13
		color 3
	]
	edge
	[
		source 11
		target 14
		color 3
	]
	edge
	[
		source 11
		target 15
		color 3
	]
	edge
	[
		source 11
		target 17
		color 3
	]
	edge
	[
		source 11
		target 19
		color 3
	]
	edge
	[
		source 11
		target 21
		color 3
	]
	edge
	[
		source 11
		target 22
		color 3
	]
	edge
	[
		source 11
		target 51
		color 3
	]
	edge
	[
		source 11
		target 53
		color 0
	]
	edge
	[
		source 11
		target 60
		color 0
	]
	edge
	[
		source 11
		target 62
		color 3
	]
	edge
	[
		source 11
		target 63
		color 3
	]
	edge
	[
		source 11
		target 66
		color 3
	]
	edge
	[
		source 11
		target 72
		color 0
	]
	edge
	[
		source 12
		target 13
		color 3
	]
	edge
	[
		source 12
		target 14
		color 3
	]
	edge
	[
		source 12
		target 15
		color 3
	]
	edge
	[
		source 12
		target 16
		color 3
	]
	edge
	[
		source 12
		target 17
		color 3
	]
	edge
	[
		source 12
		target 18
		color 3
	]
	edge
	[
		source 12
		target 19
		color 3
	]
	edge
	[
		source 12
		target 20
		color 3
	]
	edge
	[
		source 12
		target 21
		color 3
	]
	edge
	[
		source 12
		target 22
		color 3
	]
	edge
	[
		source 12
		target 23
		color 3
	]
	edge
	[
		source 12
		target 51
		color 3
	]
	edge
	[
		source 12
		target 52
		color 3
	]
	edge
	[
		source 12
		target 61
		color 3
	]
	edge
	[
		source 12
		target 62
		color 3
	]
	edge
	[
		source 12
		target 63
		color 3
	]
	edge
	[
		source 12
		target 64
		color 3
	]
	edge
	[
		source 12
		target 65
		color 3
	]
	edge
	[
		source 12
		target 66
		color 3
	]
	edge
	[
		source 12
		target 67
		color 3
	]
	edge
	[
		source 13
		target 14
		color 3
	]
	edge
	[
		source 13
		target 15
		color 3
	]
	edge
	[
		source 13
		target 16
		color 3
	]
	edge
	[
		source 13
		target 17
		color 3
	]
	edge
	[
		source 13
		target 18
		color 3
	]
	edge
	[
		source 13
		target 19
		color 3
	]
	edge
	[
		source 13
		target 20
		color 3
	]
	edge
	[
		source 13
		target 21
		color 3
	]
	edge
	[
		source 13
		target 22
		color 3
	]
	edge
	[
		source 13
		target 23
		color 3
	]
	edge
	[
		source 13
		target 51
		color 3
	]
	edge
	[
		source 13
		target 52
		color 3
	]
	edge
	[
		source 13
		target 61
		color 3
	]
	edge
	[
		source 13
		target 62
		color 3
	]
	edge
	[
		source 13
		target 63
		color 3
	]
	edge
	[
		source 13
		target 64
		color 3
	]
	edge
	[
		source 13
		target 65
		color 3
	]
	edge
	[
		source 13
		target 66
		color 3
	]
	edge
	[
		source 13
		target 67
		color 3
	]
	edge
	[
		source 14
		target 15
		color 3
	]
	edge
	[
		source 14
		target 16
		color 3
	]
	edge
	[
		source 14
		target 17
		color 3
	]
	edge
	[
		source 14
		target 18
		color 3
	]
	edge
	[
		source 14
		target 19
		color 3
	]
	edge
	[
		source 14
		target 20
		color 3
	]
	edge
	[
		source 14
		target 21
		color 3
	]
	edge
	[
		source 14
		target 22
		color 3
	]
	edge
	[
		source 14
		target 23
		color 3
	]
	edge
	[
		source 14
		target 51
		color 3
	]
	edge
	[
		source 14
		target 52
		color 3
	]
	edge
	[
		source 14
		target 62
		color 3
	]
	edge
	[
		source 14
		target 63
		color 3
	]
	edge
	[
		source 14
		target 64
		color 3
	]
	edge
	[
		source 14
		target 65
		color 3
	]
	edge
	[
		source 14
		target 66
		color 3
	]
	edge
	[
		source 14
		target 67
		color 3
	]
	edge
	[
		source 15
		target 16
		color 3
	]
	edge
	[
		source 15
		target 17
		color 3
	]
	edge
	[
		source 15
		target 18
		color 3
	]
	edge
	[
		source 15
		target 19
		color 3
	]
	edge
	[
		source 15
		target 20
		color 3
	]
	edge
	[
		source 15
		target 21
		color 3
	]
	edge
	[
		source 15
		target 22
		color 3
	]
	edge
	[
		source 15
		target 23
		color 3
	]
	edge
	[
		source 15
		target 51
		color 3
	]
	edge
	[
		source 15
		target 52
		color 3
	]
	edge
	[
		source 15
		target 61
		color 3
	]
	edge
	[
		source 15
		target 62
		color 3
	]
	edge
	[
		source 15
		target 63
		color 3
	]
	edge
	[
		source 15
		target 64
		color 3
	]
	edge
	[
		source 15
		target 65
		color 3
	]
	edge
	[
		source 15
		target 66
		color 3
	]
	edge
	[
		source 15
		target 67
		color 3
	]
	edge
	[
		source 16
		target 17
		color 3
	]
	edge
	[
		source 16
		target 18
		color 3
	]
	edge
	[
		source 16
		target 19
		color 3
	]
	edge
	[
		source 16
		target 20
		color 3
	]
	edge
	[
		source 16
		target 21
		color 3
	]
	edge
	[
		source 16
		target 22
		color 3
	]
	edge
	[
		source 16
		target 23
		color 3
	]
	edge
	[
		source 16
		target 51
		color 3
	]
	edge
	[
		source 16
		target 61
		color 3
	]
	edge
	[
		source 16
		target 62
		color 3
	]
	edge
	[
		source 16
		target 63
		color 3
	]
	edge
	[
		source 16
		target 64
		color 3
	]
	edge
	[
		source 16
		target 65
		color 3
	]
	edge
	[
		source 16
		target 66
		color 3
	]
	edge
	[
		source 16
		target 67
		color 3
	]
	edge
	[
		source 17
		target 18
		color 3
	]
	edge
	[
		source 17
		target 19
		color 3
	]
	edge
	[
		source 17
		target 20
		color 3
	]
	edge
	[
		source 17
		target 21
		color 3
	]
	edge
	[
		source 17
		target 22
		color 3
	]
	edge
	[
		source 17
		target 23
		color 3
	]
	edge
	[
		source 17
		target 51
		color 3
	]
	edge
	[
		source 17
		target 52
		color 3
	]
	edge
	[
		source 17
		target 61
		color 3
	]
	edge
	[
		source 17
		target 62
		color 3
	]
	edge
	[
		source 17
		target 63
		color 3
	]
	edge
	[
		source 17
		target 64
		color 3
	]
	edge
	[
		source 17
		target 65
		color 3
	]
	edge
	[
		source 17
		target 66
		color 3
	]
	edge
	[
		source 17
		target 67
		color 3
	]
	edge
	[
		source 18
		target 19
		color 3
	]
	edge
	[
		source 18
		target 20
		color 3
	]
	edge
	[
		source 18
		target 21
		color 3
	]
	edge
	[
		source 18
		target 22
		color 3
	]
	edge
	[
		source 18
		target 23
		color 3
	]
	edge
	[
		source 18
		target 51
		color 3
	]
	edge
	[
		source 18
		target 52
		color 3
	]
	edge
	[
		source 18
		target 61
		color 3
	]
	edge
	[
		source 18
		target 62
		color 3
	]
	edge
	[
		source 18
		target 63
		color 3
	]
	edge
	[
		source 18
		target 64
		color 3
	]
	edge
	[
		source 18
		target 65
		color 3
	]
	edge
	[
		source 18
		target 66
		color 3
	]
	edge
	[
		source 18
		target 67
		color 3
	]
	edge
	[
		source 19
		target 20
		color 3
	]
	edge
	[
		source 19
		target 21
		color 3
	]
	edge
	[
		source 19
		target 22
		color 3
	]
	edge
	[
		source 19
		target 23
		color 3
	]
	edge
	[
		source 19
		target 51
		color 3
	]
	edge
	[
		source 19
		target 52
		color 3
	]
	edge
	[
		source 19
		target 61
		color 3
	]
	edge
	[
		source 19
		target 62
		color 3
	]
	edge
	[
		source 19
		target 63
		color 3
	]
	edge
	[
		source 19
		target 64
		color 3
	]
	edge
	[
		source 19
		target 65
		color 3
	]
	edge
	[
		source 19
		target 66
		color 3
	]
	edge
	[
		source 19
		target 67
		color 3
	]
	edge
	[
		source 20
		target 21
		color 3
	]
	edge
	[
		source 20
		target 22
		color 3
	]
	edge
	[
		source 20
		target 23
		color 3
	]
	edge
	[
		source 20
		target 51
		color 3
	]
	edge
	[
		source 20
		target 52
		color 3
	]
	edge
	[
		source 20
		target 61
		color 3
	]
	edge
	[
		source 20
		target 62
		color 3
	]
	edge
	[
		source 20
		target 63
		color 3
	]
	edge
	[
		source 20
		target 64
		color 3
	]
	edge
	[
		source 20
		target 65
		color 3
	]
	edge
	[
		source 20
		target 66
		color 3
	]
	edge
	[
		source 20
		target 67
		color 3
	]
	edge
	[
		source 21
		target 22
		color 3
	]
	edge
	[
		source 21
		target 23
		color 3
	]
	edge
	[
		source 21
		target 51
		color 3
	]
	edge
	[
		source 21
		target 62
		color 3
	]
	edge
	[
		source 21
		target 63
		color 3
	]
	edge
	[
		source 21
		target 64
		color 3
	]
	edge
	[
		source 21
		target 65
		color 3
	]
	edge
	[
		source 21
		target 66
		color 3
	]
	edge
	[
		source 21
		target 67
		color 3
	]
	edge
	[
		source 22
		target 23
		color 3
	]
	edge
	[
		source 22
		target 51
		color 3
	]
	edge
	[
		source 22
		target 52
		color 3
	]
	edge
	[
		source 22
		target 62
		color 3
	]
	edge
	[
		source 22
		target 63
		color 3
	]
	edge
	[
		source 22
		target 64
		color 3
	]
	edge
	[
		source 22
		target 65
		color 3
	]
	edge
	[
		source 22
		target 66
		color 3
	]
	edge
	[
		source 22
		target 67
		color 3
	]
	edge
	[
		source 23
		target 51
		color 3
	]
	edge
	[
		source 23
		target 52
		color 3
	]
	edge
	[
		source 23
		target 61
		color 3
	]
	edge
	[
		source 23
		target 62
		color 3
	]
	edge
	[
		source 23
		target 63
		color 3
	]
	edge
	[
		source 23
		target 64
		color 3
	]
	edge
	[
		source 23
		target 65
		color 3
	]
	edge
	[
		source 23
		target 66
		color 3
	]
	edge
	[
		source 23
		target 67
		color 3
	]
	edge
	[
		source 24
		target 42
		color 0
	]
	edge
	[
		source 24
		target 53
		color 0
	]
	edge
	[
		source 24
		target 54
		color 0
	]
	edge
	[
		source 24
		target 55
		color 0
	]
	edge
	[
		source 24
		target 60
		color 0
	]
	edge
	[
		source 24
		target 70
		color 0
	]
	edge
	[
		source 24
		target 71
		color 0
	]
	edge
	[
		source 24
		target 72
		color 0
	]
	edge
	[
		source 24
		target 73
		color 0
	]
	edge
	[
		source 24
		target 74
		color 0
	]
	edge
	[
		source 25
		target 26
		color 2
	]
	edge
	[
		source 25
		target 27
		color 2
	]
	edge
	[
		source 25
		target 28
		color 2
	]
	edge
	[
		source 25
		target 29
		color 2
	]
	edge
	[
		source 25
		target 30
		color 2
	]
	edge
	[
		source 25
		target 31
		color 2
	]
	edge
	[
		source 25
		target 32
		color 2
	]
	edge
	[
		source 25
		target 33
		color 2
	]
	edge
	[
		source 25
		target 35
		color 2
	]
	edge
	[
		source 25
		target 36
		color 2
	]
	edge
	[
		source 26
		target 27
		color 2
	]
	edge
	[
		source 26
		target 28
		color 2
	]
	edge
	[
		source 26
		target 29
		color 2
	]
	edge
	[
		source 26
		target 30
		color 2
	]
	edge
	[
		source 26
		target 31
		color 2
	]
	edge
	[
		source 26
		target 32
		color 2
	]
	edge
	[
		source 26
		target 33
		color 2
	]
	edge
	[
		source 26
		target 35
		color 2
	]
	edge
	[
		source 26
		target 36
		color 2
	]
	edge
	[
		source 27
		target 28
		color 2
	]
	edge
	[
		source 27
		target 29
		color 2
	]
	edge
	[
		source 27
		target 30
		color 2
	]
	edge
	[
		source 27
		target 31
		color 2
	]
	edge
	[
		source 27
		target 35
		color 2
	]
	edge
	[
		source 27
		target 36
		color 2
	]
	edge
	[
		source 28
		target 29
		color 2
	]
	edge
	[
		source 28
		target 30
		color 2
	]
	edge
	[
		source 28
		target 31
		color 2
	]
	edge
	[
		source 28
		target 35
		color 2
	]
	edge
	[
		source 28
		target 37
		color 1
	]
	edge
	[
		source 28
		target 39
		color 1
	]
	edge
	[
		source 28
		target 40
		color 1
	]
	edge
	[
		source 28
		target 41
		color 1
	]
	edge
	[
		source 28
		target 43
		color 1
	]
	edge
	[
		source 28
		target 44
		color 1
	]
	edge
	[
		source 28
		target 45
		color 1
	]
	edge
	[
		source 28
		target 47
		color 1
	]
	edge
	[
		source 28
		target 48
		color 1
	]
	edge
	[
		source 28
		target 49
		color 1
	]
	edge
	[
		source 28
		target 56
		color 1
	]
	edge
	[
		source 28
		target 57
		color 1
	]
	edge
	[
		source 28
		target 59
		color 1
	]
	edge
	[
		source 28
		target 61
		color 1
	]
	edge
	[
		source 28
		target 68
		color 1
	]
	edge
	[
		source 29
		target 30
		color 2
	]
	edge
	[
		source 29
		target 31
		color 2
	]
	edge
	[
		source 29
		target 32
		color 2
	]
	edge
	[
		source 29
		target 35
		color 2
	]
	edge
	[
		source 30
		target 31
		color 2
	]
	edge
	[
		source 30
		target 32
		color 2
	]
	edge
	[
		source 30
		target 35
		color 2
	]
	edge
	[
		source 30
		target 36
		color 2
	]
	edge
	[
		source 31
		target 32
		color 2
	]
	edge
	[
		source 31
		target 35
		color 2
	]
	edge
	[
		source 32
		target 33
		color 2
	]
	edge
	[
		source 32
		target 35
		color 2
	]
	edge
	[
		source 32
		target 41
		color 1
	]
	edge
	[
		source 32
		target 45
		color 1
	]
	edge
	[
		source 32
		target 48
		color 1
	]
	edge
	[
		source 32
		target 49
		color 1
	]
	edge
	[
		source 32
		target 56
		color 1
	]
	edge
	[
		source 32
		target 57
		color 1
	]
	edge
	[
		source 32
		target 58
		color 1
	]
	edge
	[
		source 32
		target 59
		color 1
	]
	edge
	[
		source 32
		target 61
		color 1
	]
	edge
	[
		source 32
		target 68
		color 1
	]
	edge
	[
		source 33
		target 35
		color 2
	]
	edge
	[
		source 33
		target 38
		color 0
	]
	edge
	[
		source 33
		target 53
		color 0
	]
	edge
	[
		source 33
		target 60
		color 0
	]
	edge
	[
		source 33
		target 73
		color 0
	]
	edge
	[
		source 33
		target 74
		color 0
	]
	edge
	[
		source 34
		target 37
		color 1
	]
	edge
	[
		source 34
		target 38
		color 1
	]
	edge
	[
		source 34
		target 39
		color 1
	]
	edge
	[
		source 34
		target 40
		color 1
	]
	edge
	[
		source 34
		target 41
		color 1
	]
	edge
	[
		source 34
		target 42
		color 1
	]
	edge
	[
		source 34
		target 43
		color 1
	]
	edge
	[
		source 34
		target 44
		color 1
	]
	edge
	[
		source 34
		target 45
		color 1
	]
	edge
	[
		source 34
		target 46
		color 1
	]
	edge
	[
		source 34
		target 47
		color 1
	]
	edge
	[
		source 34
		target 48
		color 1
	]
	edge
	[
		source 34
		target 49
		color 1
	]
	edge
	[
		source 34
		target 50
		color 1
	]
	edge
	[
		source 34
		target 56
		color 1
	]
	edge
	[
		source 34
		target 57
		color 1
	]
	edge
	[
		source 34
		target 58
		color 1
	]
	edge
	[
		source 34
		target 59
		color 1
	]
	edge
	[
		source 34
		target 61
		color 1
	]
	edge
	[
		source 34
		target 68
		color 1
	]
	edge
	[
		source 34
		target 69
		color 1
	]
	edge
	[
		source 34
		target 70
		color 1
	]
	edge
	[
		source 35
		target 36
		color 2
	]
	edge
	[
		source 36
		target 40
		color 1
	]
	edge
	[
		source 36
		target 41
		color 1
	]
	edge
	[
		source 36
		target 44
		color 1
	]
	edge
	[
		source 36
		target 47
		color 1
	]
	edge
	[
		source 36
		target 48
		color 1
	]
	edge
	[
		source 36
		target 49
		color 1
	]
	edge
	[
		source 36
		target 58
		color 1
	]
	edge
	[
		source 37
		target 39
		color 1
	]
	edge
	[
		source 37
		target 40
		color 1
	]
	edge
	[
		source 37
		target 41
		color 1
	]
	edge
	[
		source 37
		target 43
		color 1
	]
	edge
	[
		source 37
		target 44
		color 1
	]
	edge
	[
		source 37
		target 45
		color 1
	]
	edge
	[
		source 37
		target 46
		color 1
	]
	edge
	[
		source 37
		target 47
		color 1
	]
	edge
	[
		source 37
		target 48
		color 1
	]
	edge
	[
		source 37
		target 49
		color 1
	]
	edge
	[
		source 37
		target 50
		color 1
	]
	edge
	[
		source 37
		target 56
		color 1
	]
	edge
	[
		source 37
		target 57
		color 1
	]
	edge
	[
		source 37
		target 58
		color 1
	]
	edge
	[
		source 37
		target 59
		color 1
	]
	edge
	[
		source 37
		target 61
		color 1
	]
	edge
	[
		source 37
		target 68
		color 1
	]
	edge
	[
		source 37
		target 69
		color 1
	]
	edge
	[
		source 37
		target 70
		color 1
	]
	edge
	[
		source 38
		target 39
		color 1
	]
	edge
	[
		source 38
		target 43
		color 1
	]
	edge
	[
		source 38
		target 46
		color 1
	]
	edge
	[
		source 38
		target 47
		color 1
	]
	edge
	[
		source 38
		target 48
		color 1
	]
	edge
	[
		source 38
		target 49
		color 1
	]
	edge
	[
		source 38
		target 53
		color 0
	]
	edge
	[
		source 38
		target 54
		color 0
	]
	edge
	[
		source 38
		target 55
		color 0
	]
	edge
	[
		source 38
		target 60
		color 0
	]
	edge
	[
		source 38
		target 61
		color 1
	]
	edge
	[
		source 38
		target 68
		color 1
	]
	edge
	[
		source 38
		target 72
		color 0
	]
	edge
	[
		source 38
		target 73
		color 0
	]
	edge
	[
		source 39
		target 40
		color 1
	]
	edge
	[
		source 39
		target 41
		color 1
	]
	edge
	[
		source 39
		target 42
		color 1
	]
	edge
	[
		source 39
		target 43
		color 1
	]
	edge
	[
		source 39
		target 44
		color 1
	]
	edge
	[
		source 39
		target 45
		color 1
	]
	edge
	[
		source 39
		target 46
		color 1
	]
	edge
	[
		source 39
		target 47
		color 1
	]
	edge
	[
		source 39
		target 48
		color 1
	]
	edge
	[
		source 39
		target 49
		color 1
	]
	edge
	[
		source 39
		target 50
		color 1
	]
	edge
	[
		source 39
		target 56
		color 1
	]
	edge
	[
		source 39
		target 57
		color 1
	]
	edge
	[
		source 39
		target 58
		color 1
	]
	edge
	[
		source 39
		target 59
		color 1
	]
	edge
	[
		source 39
		target 61
		color 1
	]
	edge
	[
		source 39
		target 68
		color 1
	]
	edge
	[
		source 40
		target 41
		color 1
	]
	edge
	[
		source 40
		target 42
		color 1
	]
	edge
	[
		source 40
		target 43
		color 1
	]
	edge
	[
		source 40
		target 44
		color 1
	]
	edge
	[
		source 40
		target 45
		color 1
	]
	edge
	[
		source 40
		target 46
		color 1
	]
	edge
	[
		source 40
		target 47
		color 1
	]
	edge
	[
		source 40
		target 48
		color 1
	]
	edge
	[
		source 40
		target 49
		color 1
	]
	edge
	[
		source 40
		target 50
		color 1
	]
	edge
	[
		source 40
		target 56
		color 1
	]
	edge
	[
		source 40
		target 57
		color 1
	]
	edge
	[
		source 40
		target 58
		color 1
	]
	edge
	[
		source 40
		target 59
		color 1
	]
	edge
	[
		source 40
		target 68
		color 1
	]
	edge
	[
		source 40
		target 69
		color 1
	]
	edge
	[
		source 41
		target 42
		color 1
	]
	edge
	[
		source 41
		target 43
		color 1
	]
	edge
	[
		source 41
		target 44
		color 1
	]
	edge
	[
		source 41
		target 45
		color 1
	]
	edge
	[
		source 41
		target 46
		color 1
	]
	edge
	[
		source 41
		target 47
		color 1
	]
	edge
	[
		source 41
		target 48
		color 1
	]
	edge
	[
		source 41
		target 49
		color 1
	]
	edge
	[
		source 41
		target 50
		color 1
	]
	edge
	[
		source 41
		target 56
		color 1
	]
	edge
	[
		source 41
		target 57
		color 1
	]
	edge
	[
		source 41
		target 58
		color 1
	]
	edge
	[
		source 41
		target 59
		color 1
	]
	edge
	[
		source 41
		target 61
		color 1
	]
	edge
	[
		source 41
		target 68
		color 1
	]
	edge
	[
		source 41
		target 70
		color 1
	]
	edge
	[
		source 42
		target 47
		color 1
	]
	edge
	[
		source 42
		target 50
		color 1
	]
	edge
	[
		source 42
		target 53
		color 0
	]
	edge
	[
		source 42
		target 54
		color 0
	]
	edge
	[
		source 42
		target 55
		color 0
	]
	edge
	[
		source 42
		target 57
		color 1
	]
	edge
	[
		source 42
		target 59
		color 1
	]
	edge
	[
		source 42
		target 60
		color 0
	]
	edge
	[
		source 42
		target 72
		color 0
	]
	edge
	[
		source 42
		target 73
		color 0
	]
	edge
	[
		source 42
		target 74
		color 0
	]
	edge
	[
		source 43
		target 45
		color 1
	]
	edge
	[
		source 43
		target 46
		color 1
	]
	edge
	[
		source 43
		target 47
		color 1
	]
	edge
	[
		source 43
		target 48
		color 1
	]
	edge
	[
		source 43
		target 49
		color 1
	]
	edge
	[
		source 43
		target 50
		color 1
	]
	edge
	[
		source 43
		target 56
		color 1
	]
	edge
	[
		source 43
		target 57
		color 1
	]
	edge
	[
		source 43
		target 58
		color 1
	]
	edge
	[
		source 43
		target 59
		color 1
	]
	edge
	[
		source 43
		target 61
		color 1
	]
	edge
	[
		source 43
		target 68
		color 1
	]
	edge
	[
		source 43
		target 69
		color 1
	]
	edge
	[
		source 43
		target 70
		color 1
	]
	edge
	[
		source 44
		target 45
		color 1
	]
	edge
	[
		source 44
		target 46
		color 1
	]
	edge
	[
		source 44
		target 47
		color 1
	]
	edge
	[
		source 44
		target 48
		color 1
	]
	edge
	[
		source 44
		target 49
		color 1
	]
	edge
	[
		source 44
		target 50
		color 1
	]
	edge
	[
		source 44
		target 54
		color 0
	]
	edge
	[
		source 44
		target 56
		color 1
	]
	edge
	[
		source 44
		target 57
		color 1
	]
	edge
	[
		source 44
		target 58
		color 1
	]
	edge
	[
		source 44
		target 61
		color 1
	]
	edge
	[
		source 44
		target 68
		color 1
	]
	edge
	[
		source 45
		target 46
		color 1
	]
	edge
	[
		source 45
		target 47
		color 1
	]
	edge
	[
		source 45
		target 48
		color 1
	]
	edge
	[
		source 45
		target 49
		color 1
	]
	edge
	[
		source 45
		target 50
		color 1
	]
	edge
	[
		source 45
		target 56
		color 1
	]
	edge
	[
		source 45
		target 57
		color 1
	]
	edge
	[
		source 45
		target 58
		color 1
	]
	edge
	[
		source 45
		target 59
		color 1
	]
	edge
	[
		source 45
		target 61
		color 1
	]
	edge
	[
		source 45
		target 68
		color 1
	]
	edge
	[
		source 45
		target 69
		color 1
	]
	edge
	[
		source 46
		target 47
		color 1
	]
	edge
	[
		source 46
		target 48
		color 1
	]
	edge
	[
		source 46
		target 49
		color 1
	]
	edge
	[
		source 46
		target 50
		color 1
	]
	edge
	[
		source 46
		target 56
		color 1
	]
	edge
	[
		source 46
		target 57
		color 1
	]
	edge
	[
		source 46
		target 58
		color 1
	]
	edge
	[
		source 46
		target 59
		color 1
	]
	edge
	[
		source 46
		target 61
		color 1
	]
	edge
	[
		source 46
		target 68
		color 1
	]
	edge
	[
		source 47
		target 48
		color 1
	]
	edge
	[
		source 47
		target 49
		color 1
	]
	edge
	[
		source 47
		target 50
		color 1
	]
	edge
	[
		source 47
		target 56
		color 1
	]
	edge
	[
		source 47
		target 57
		color 1
	]
	edge
	[
		source 47
		target 58
		color 1
	]
	edge
	[
		source 47
		target 59
		color 1
	]
	edge
	[
		source 47
		target 61
		color 1
	]
	edge
	[
		source 47
		target 68
		color 1
	]
	edge
	[
		source 47
		target 69
		color 1
	]
	edge
	[
		source 47
		target 70
		color 1
	]
	edge
	[
		source 48
		target 49
		color 1
	]
	edge
	[
		source 48
		target 50
		color 1
	]
	edge
	[
		source 48
		target 56
		color 1
	]
	edge
	[
		source 48
		target 57
		color 1
	]
	edge
	[
		source 48
		target 58
		color 1
	]
	edge
	[
		source 48
		target 59
		color 1
	]
	edge
	[
		source 48
		target 61
		color 1
	]
	edge
	[
		source 48
		target 68
		color 1
	]
	edge
	[
		source 48
		target 70
		color 1
	]
	edge
	[
		source 49
		target 50
		color 1
	]
	edge
	[
		source 49
		target 56
		color 1
	]
	edge
	[
		source 49
		target 57
		color 1
	]
	edge
	[
		source 49
		target 58
		color 1
	]
	edge
	[
		source 49
		target 59
		color 1
	]
	edge
	[
		source 49
		target 68
		color 1
	]
	edge
	[
		source 49
		target 69
		color 1
	]
	edge
	[
		source 50
		target 56
		color 1
	]
	edge
	[
		source 50
		target 57
		color 1
	]
	edge
	[
		source 50
		target 58
		color 1
	]
	edge
	[
		source 50
		target 59
		color 1
	]
	edge
	[
		source 50
		target 61
		color 1
	]
	edge
	[
		source 50
		target 63
		color 1
	]
	edge
	[
		source 50
		target 68
		color 1
	]
	edge
	[
		source 50
		target 70
		color 1
	]
	edge
	[
		source 51
		target 52
		color 3
	]
	edge
	[
		source 51
		target 61
		color 3
	]
	edge
	[
		source 51
		target 62
		color 3
	]
	edge
	[
		source 51
		target 63
		color 3
	]
	edge
	[
		source 51
		target 64
		color 3
	]
	edge
	[
		source 51
		target 65
		color 3
	]
	edge
	[
		source 51
		target 66
		color 3
	]
	edge
	[
		source 51
		target 67
		color 3
	]
	edge
	[
		source 52
		target 62
		color 3
	]
	edge
	[
		source 52
		target 63
		color 3
	]
	edge
	[
		source 52
		target 64
		color 3
	]
	edge
	[
		source 52
		target 66
		color 3
	]
	edge
	[
		source 52
		target 67
		color 3
	]
	edge
	[
		source 52
		target 72
		color 0
	]
	edge
	[
		source 53
		target 54
		color 0
	]
	edge
	[
		source 53
		target 55
		color 0
	]
	edge
	[
		source 53
		target 60
		color 0
	]
	edge
	[
		source 53
		target 70
		color 0
	]
	edge
	[
		source 53
		target 71
		color 0
	]
	edge
	[
		source 53
		target 72
		color 0
	]
	edge
	[
		source 53
		target 73
		color 0
	]
	edge
	[
		source 53
		target 74
		color 0
	]
	edge
	[
		source 54
		target 55
		color 0
	]
	edge
	[
		source 54
		target 60
		color 0
	]
	edge
	[
		source 54
		target 71
		color 0
	]
	edge
	[
		source 54
		target 72
		color 0
	]
	edge
	[
		source 54
		target 73
		color 0
	]
	edge
	[
		source 54
		target 74
		color 0
	]
	edge
	[
		source 55
		target 60
		color 0
	]
	edge
	[
		source 55
		target 71
		color 0
	]
	edge
	[
		source 55
		target 72
		color 0
	]
	edge
	[
		source 55
		target 73
		color 0
	]
	edge
	[
		source 55
		target 74
		color 0
	]
	edge
	[
		source 56
		target 57
		color 1
	]
	edge
	[
		source 56
		target 58
		color 1
	]
	edge
	[
		source 56
		target 59
		color 1
	]
	edge
	[
		source 56
		target 61
		color 1
	]
	edge
	[
		source 56
		target 68
		color 1
	]
	edge
	[
		source 56
		target 69
		color 1
	]
	edge
	[
		source 56
		target 70
		color 1
	]
	edge
	[
		source 57
		target 58
		color 1
	]
	edge
	[
		source 57
		target 59
		color 1
	]
	edge
	[
		source 57
		target 61
		color 1
	]
	edge
	[
		source 57
		target 68
		color 1
	]
	edge
	[
		source 57
		target 69
		color 1
	]
	edge
	[
		source 58
		target 59
		color 1
	]
	edge
	[
		source 58
		target 61
		color 1
	]
	edge
	[
		source 58
		target 68
		color 1
	]
	edge
	[
		source 58
		target 69
		color 1
	]
	edge
	[
		source 58
		target 70
		color 1
	]
	edge
	[
		source 59
		target 61
		color 1
	]
	edge
	[
		source 59
		target 68
		color 1
	]
	edge
	[
		source 59
		target 69
		color 1
	]
	edge
	[
		source 60
		target 71
		color 0
	]
	edge
	[
		source 60
		target 72
		color 0
	]
	edge
	[
		source 60
		target 73
		color 0
	]
	edge
	[
		source 60
		target 74
		color 0
	]
	edge
	[
		source 61
		target 62
		color 3
	]
	edge
	[
		source 61
		target 63
		color 3
	]
	edge
	[
		source 61
		target 64
		color 3
	]
	edge
	[
		source 61
		target 65
		color 3
	]
	edge
	[
		source 61
		target 66
		color 3
	]
	edge
	[
		source 61
		target 67
		color 3
	]
	edge
	[
		source 61
		target 68
		color 1
	]
	edge
	[
		source 61
		target 69
		color 1
	]
	edge
	[
		source 62
		target 64
		color 3
	]
	edge
	[
		source 62
		target 65
		color 3
	]
	edge
	[
		source 62
		target 66
		color 3
	]
	edge
	[
		source 62
		target 67
		color 3
	]
	edge
	[
		source 63
		target 64
		color 3
	]
	edge
	[
		source 63
		target 65
		color 3
	]
	edge
	[
		source 63
		target 66
		color 3
	]
	edge
	[
		source 63
		target 67
		color 3
	]
	edge
	[
		source 64
		target 65
		color 3
	]
	edge
	[
		source 64
		target 66
		color 3
	]
	edge
	[
		source 64
		target 67
		color 3
	]
	edge
	[
		source 65
		target 66
		color 3
	]
	edge
	[
		source 65
		target 67
		color 3
	]
	edge
	[
		source 66
		target 67
		color 3
	]
	edge
	[
		source 68
		target 69
		color 1
	]
	edge
	[
		source 68
		target 70
		color 1
	]
	edge
	[
		source 70
		target 74
		color 0
	]
	edge
	[
		source 71
		target 72
		color 0
	]
	edge
	[
		source 71
		target 73
		color 0
	]
	edge
	[
		source 71
		target 74
		color 0
	]
	edge
	[
		source 72
		target 73
		color 0
	]
	edge
	[
		source 72
		target 74
		color 0
	]
	edge
	[
		source 73
		target 74
		color 0
	]
